#!/usr/bin/env python3
"""Benchmark of the pseudo-label hot path (BASELINE.json metric: pseudo-labeled LiDAR frames/sec,
150k-pt frames, ~60 clusters, at 1/2/4/8 MI355X).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...          (without a launcher: bench.py starts the N ranks itself, as child processes)

A "step" = one synthetic 150k-point frame through the whole per-frame path (ground removal -> ref transform -> HDBSCAN ->
filters -> multi-view render -> CLIP ViT-B/16 fp16 encode -> scores -> vote -> boxes -> result dict).  Weak scaling: ONE
sequence of N*K frames is sharded over the N ranks.  Patchwork++'s adaptive state runs through the whole sequence (the sensor height
estimated on frame i seeds frame i + 1): by default (`--ground-handoff replicate`) the frames are dealt ROUND-ROBIN (frame g -> rank
g % N) and every rank runs the cheap stateful ground pass over all N*K frames itself, on its high-priority stream under its own
frames' ViT work -- rank r's first frame waits for r ground passes (0.36 ms each) and nothing is exchanged; `chain` shards contiguous
blocks of K frames like the stage dispatcher (vilgod_amd/zero_shot_detector.py, vilgod_amd/dist.py) and hands the state down the rank
chain (vg_ground_export_state / vg_ground_set_state: rank r starts r*K passes late), `replay` re-runs the ground stage over the r*K
frames before the block.  All inside the timed region.  The only data-path collective is ONE all-gather of the per-crop score matrices after the K
frames (north_star).  The run is a real stream: every one of the W + K frames of a rank is a DISTINCT seeded synthetic cloud (no
cycling -- a new crop count almost every frame), handed over as a pinned HOST buffer (SURVEY 8d's clock: "raw points resident in
host pinned memory" to "result dict on the host"; the copy to HBM is queued inside the timed region; `--input resident` uploads
the K clouds before the clock starts instead and is reported as the `resident_input` block).  Each rank keeps `--inflight` frames
(default 6) in flight on worker threads with their own streams and handles.  Before the W warm-up steps an untimed set-up block
of min(K, 24) further distinct clouds brings the caching allocator -- and a freshly leased box's first second of GPU load -- to the
steady state of a long-running stream: at least three passes, repeated until two agree within 3 %, at most 8 times (config.setup_frames = frames
run that way; not steps of the metric).  The ViT runs as plain stream launches (default) or
as captured hipGraphs per crop-count bucket (`--vit-graph`; captures then happen INSIDE the timed region and are counted in
`config.graphs_captured`).  The K timed frames include filling and draining the pipeline (small K therefore reads a little
lower: the driver's K = 20 run vs the default K = 96).  `--steps` is the number of timed steps: by default ONE timed block of K steps
(`ms_per_step` = its time / K).  `--blocks B` splits the K steps into B blocks of K / B steps each, every block on its own distinct clouds
and bracketed by its own barrier + synchronize; `value` is then the MEDIAN block (`block_values`, `block_spread`; `ms_per_step` = the
median block's time / its steps): one 0.3 s window on a shared box reads +-4 %.  `--dump-outputs DIR` writes what the last timed step
returned (result dict, FrameState arrays, score matrix) as DIR/<name>.npy after the timed steps: the inputs are seeded, so two builds
run with the same arguments can be compared output for output.

A plain run does only what the metric needs: set-up, warm-up, the timed steps, `--dump-outputs`, the JSON line.  Everything else
runs after the timed steps and only with `--full` (the `--no-*` switches below then leave out single parts of it).  With `--full`
the JSON line also carries
  roofline      the dominant kernel (the ViT projection GEMM): algorithmic FLOPs / launch duration, measured live with HIP
                event pairs on the launch stream (csrc/vit.hip vg_vit_profile), vs the dense fp16 MFMA peak of the MI355X
                (PEAK_F16_MFMA_TFLOPS); tower_two_in_flight and frame_latency_ms beside it
  cpu_baseline  the CPU oracle (oracle/pipeline_oracle.py, kind "port": the reference cannot travel to the GPU box) timed on a
                bounded sample of the metric's workload on the host cores of the same box (rank 0, N=1 only)
and, as information beside the metric (N=1 only; each block reports its own failure instead of costing the metric line):
  multi_gpu_model      what frame sharding costs, modelled and emulated as rank 0 of N on this one GPU
  box_modes            the same frames with box_mode 'fast' (GPU hull, all edges) next to the default 'reference' mode
  resident_input       the same frames uploaded to HBM before the clock starts (what rounds 1-2 quoted as the metric)
  resid16              the same frames with the fp16 residual stream of the reference's own GPU run (VG_VIT_RESID16=1) beside the default fp32 stream
  hipgraph_loop        the same frames with the ViT as captured hipGraphs (per crop-count bucket, LRU-bounded) next to the default plain launches
  views6, dense200k    BASELINE configs 3 (6 rendered views) and 5 (200k points, ~120 objects) shapes
  default_config_mode  the reference's default stage order -- entropy scores + two-frame clustering -- as a library call
  cli_mode             tools/preprocess_data.py itself: the default 9-stage list on four 199-frame 150k-point synthetic sequences (steady state of a multi-sequence run)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')      # one hardware queue per stream in flight (vilgod_amd/__init__.py), before the runtime starts

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VIT_FLOP_PER_CROP = 2 * 17_563_453_440
PEAK_F16_MFMA_TFLOPS = 2500.0                   # MI355X_MICROARCH.md: ~2.5 PF dense fp16/bf16
DOMINANT_KERNEL = 'k_gemm_f16_pp64' if os.environ.get('VG_GEMM_W4') == '0' else 'k_gemm_f16_w4'


def cpu_baseline(n_points=150_000, n_objects=60, vit_crops=32, with_20k=True):
    """Whole path on the host cores on a BOUNDED sample of the metric's workload: ONE 150k-point frame through every stage, the
    ViT (the dominant CPU cost, linear in the crops) on the first `vit_crops` crops and extrapolated to the frame's crops."""
    import torch
    from oracle.pipeline_oracle import OraclePipeline
    from oracle import vit_oracle as vo
    from vilgod_amd import synthetic, clip_weights as cw
    from vilgod_amd.pipeline import default_preprocessor_cfg
    # SURVEY 8d asks for the host's cores.  Measured on the GPU box (2 x EPYC 9575F, 256 logical CPUs, round 4): with 256 torch threads the
    # ViT leg runs 12x SLOWER than with 16 (490 s instead of ~40 s per 150k-point frame) and the stages made of thousands of small tensor
    # ops (renderer, clustering glue) 20x slower -- oversubscription, not work.  A baseline that handicaps the CPU would flatter the GPU, so
    # the ViT leg -- ~97 % of the CPU time -- runs on the thread count that is FASTEST on this host (a few crops timed at 16, 32, 64, 128
    # and all logical CPUs; `cores` = the winner), the small-op stages on at most 16.
    n_small = min(16, os.cpu_count())
    torch.set_num_threads(n_small)
    host_model = 'unknown'
    try:
        with open('/proc/cpuinfo') as f:
            host_model = next((ln.split(':', 1)[1].strip() for ln in f if ln.startswith('model name')), 'unknown')
    except OSError:
        pass
    cfg = default_preprocessor_cfg()
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    text = cw.synthetic_text_features(0, 24, 512)
    orc = OraclePipeline(wd, text, cfg['clip']['class_list'], cfg['clip']['class_mapping'], clusterer='sklearn', box_all_edges=False)
    cal = {}
    xc = torch.randn(4, 3, 224, 224)
    for nt in sorted({t for t in (16, 32, 64, 128, os.cpu_count()) if t <= os.cpu_count()}):
        torch.set_num_threads(nt)
        vo.encode_in_chunks(wd, xc[:1], 12, 64)
        t0 = time.perf_counter()
        vo.encode_in_chunks(wd, xc, 12, 64)
        cal[nt] = time.perf_counter() - t0
        if cal[nt] > 3.0 * min(cal.values()):           # past the optimum (256 threads: 40 s for these four crops): stop climbing
            break
    n_threads = min(cal, key=cal.get)
    torch.set_num_threads(n_small)
    poses = synthetic.make_poses(4)
    out = {}

    def run(points, objects, n_frames, crop_cap):
        frames = [synthetic.make_frame(1000 + i, points, n_objects=objects) for i in range(n_frames)]
        orig = vo.encode_in_chunks
        seen = {'crops': 0, 'encoded': 0, 'vit_s': 0.0}

        def capped(wd_, x, heads, chunk):
            # time the tower on at most crop_cap crops, return features for all (the rest repeats the last one: only the
            # timing is used below, never the classes)
            n = len(x)
            k = n if crop_cap is None else min(n, crop_cap)
            torch.set_num_threads(n_threads)
            t0 = time.perf_counter()
            f = orig(wd_, x[:k], heads, chunk)
            seen['vit_s'] += time.perf_counter() - t0
            torch.set_num_threads(n_small)
            seen['crops'] += n
            seen['encoded'] += k
            return f if k == n else torch.cat([f, f[-1:].expand(n - k, -1)])
        vo.encode_in_chunks = capped
        try:
            t0 = time.perf_counter()
            valid = 0
            tsum = {}
            for i in range(n_frames):
                o = orc.process_frame(frames[i], poses[i + 1], poses[0])
                valid += int(o['valid'].sum())
                for k, v in orc.timings.items():
                    tsum[k] = tsum.get(k, 0.0) + v
            dt = time.perf_counter() - t0
        finally:
            vo.encode_in_chunks = orig
        vit_full = seen['vit_s'] * seen['crops'] / max(seen['encoded'], 1)
        tsum['vit'] = tsum.get('vit', 0.0) - seen['vit_s'] + vit_full           # the 'vit' tick also holds scores/top-1 (negligible)
        total = dt - seen['vit_s'] + vit_full
        return total, dt, valid, seen, tsum

    orc.new_sequence()
    total, dt, valid, seen, tsum = run(n_points, n_objects, 1, vit_crops)
    out = {
        'value': round(1.0 / total, 5), 'unit': 'frames/s', 'cores': n_threads, 'kind': 'port',
        'host': {'cpu_count': os.cpu_count(), 'model': host_model, 'torch_threads_vit': n_threads, 'torch_threads_other_stages': n_small,
                 'vit_seconds_for_4_crops_by_threads': {str(k): round(v, 2) for k, v in cal.items()}},
        'sample': (f'ONE synthetic frame of {n_points} points (the metric\'s workload; {valid} valid clusters, {seen["crops"]} crops) through '
                   f'all stages in {dt:.1f} s of CPU work; the ViT was run on the first {seen["encoded"]} crops ({seen["vit_s"]:.1f} s) and '
                   f'extrapolated linearly to all {seen["crops"]} (-> {total:.1f} s per frame): ' + ', '.join(f'{k} {v:.2f}s' for k, v in tsum.items()) +
                   '; clustering = sklearn.cluster.HDBSCAN stand-in (the reference\'s hdbscan package is absent; its Boruvka is '
                   'faster than this Prim), ViT = torch-CPU fp32, same synthetic weights; boxes = scipy qhull + numpy like the reference'),
    }
    if with_20k:
        orc.new_sequence()
        total2, dt2, valid2, seen2, tsum2 = run(20_000, 8, 3, None)
        out['config0_20k'] = {'value': round(3 / total2, 5), 'unit': 'frames/s (20k-pt frames)',
                              'sample': f'3 consecutive synthetic frames of 20000 points, everything run ({valid2} valid clusters, '
                                        f'{seen2["crops"]} crops, {dt2:.1f} s): ' + ', '.join(f'{k} {v:.2f}s' for k, v in tsum2.items())}
    return out


def dump_outputs(out_dir, step, class_names):
    """`--dump-outputs`: what a caller of the timed path receives for one step (its FrameState, result dict and per-crop score
    matrix) as out_dir/<name>.npy, float64 (float32 for the scores the GPU computes in float32).  Class names are stored as their index
    into `class_names`; the ground set is sorted (it is a set); `boxes_ref` holds the boxes of the valid clusters only (the others have
    none: NaN rows in FrameState.boxes), in cluster order.  A 150k-point frame writes about 1.2 MB."""
    fs, res, probs = step
    index = {str(n): i for i, n in enumerate(class_names)}
    arrays = {
        'boxes_lidar': np.asarray(res['boxes_lidar'], np.float64).reshape(-1, 7),
        'class_index': np.array([index[str(n)] for n in res['name']], np.float64),
        'score': np.asarray(res['score'], np.float64),
        'moving': np.asarray(res['moving'], np.float64),
        'crop_probs': probs.float().cpu().numpy(),
        'ground_point_indices': np.sort(np.asarray(fs.ground_point_indices)).astype(np.float64),
        'cluster_ids': np.asarray(fs.cluster_ids, np.float64),
        'cluster_valid': np.asarray(fs.valid, np.float64),
        'cluster_point_index': np.asarray(fs.index, np.float64),
        'cluster_point_offsets': np.asarray(fs.seg_off, np.float64),
        'boxes_ref': np.zeros((0, 7)) if fs.boxes is None else np.asarray(fs.boxes, np.float64)[np.asarray(fs.valid, bool)],
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes (nothing here has touched the GPU) through
    torch.distributed.run and pass their output through."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=96)
    ap.add_argument('--warmup', type=int, default=12)
    ap.add_argument('--blocks', type=int, default=1, help='split the --steps timed steps into this many blocks of equal length, on distinct clouds, '
                    'every one bracketed by its own barrier + synchronize; value = the MEDIAN block (one 0.3 s window on a shared box reads +-4 %%)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32 / float64)')
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--dtype', default='f16', choices=['f16', 'f32'])
    ap.add_argument('--box-mode', default='reference', choices=['reference', 'fast'])
    ap.add_argument('--ground-handoff', default='replicate', choices=['replicate', 'relay', 'chain', 'replay'],
                    help='N > 1: how a rank obtains the Patchwork++ state its frames need (inside the timed region).  replicate (default): '
                         'frames dealt round-robin, every rank runs the ground pass over the whole sequence itself, nothing is exchanged; '
                         'chain / replay: contiguous blocks, state handed down the rank chain / ground passes of the earlier blocks replayed')
    ap.add_argument('--vit-graph', action='store_true', help='captured hipGraphs (one per crop-count bucket and worker, LRU-bounded) for the ViT instead of plain stream launches')
    ap.add_argument('--input', default='host', choices=['host', 'resident'],
                    help='host: every frame is handed over as a pinned host buffer, H2D inside the timed region (SURVEY 8d); resident: uploaded before the clock starts')
    ap.add_argument('--angle-mode', default='reference', choices=['device', 'reference'], help='view angle of a cluster: on the GPU, or by this host\'s numpy (projection.py)')
    ap.add_argument('--emulate-world', type=int, nargs='*', default=[2, 4, 8],
                    help='N = 1 only: world sizes whose rank 0 this one GPU emulates inside the multi_gpu_model block (all N K uploads + ground '
                         'passes of the replicated round-robin design, K own frames); empty = skip')
    ap.add_argument('--full', action='store_true', help='after the timed steps, also measure everything beside the metric: roofline pass, frame latency, '
                    'information blocks, reference stage order, cli_mode, CPU baseline (off: the run does only what the metric line needs)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-extras', action='store_true', help='skip the information blocks beside the metric (box_modes, views6, dense200k, cli_mode)')
    ap.add_argument('--cli-frames', type=int, default=199, help='frames of the synthetic sequence of the cli_mode block')
    ap.add_argument('--cli-sequences', type=int, default=4, help='sequences of the cli_mode block (the same world under several names)')
    ap.add_argument('--stage-times', action='store_true', help='print per-stage ms (adds synchronisation; not for the metric)')
    ap.add_argument('--no-roofline-pass', action='store_true', help='skip the sequential GEMM-timing pass (profiling runs)')
    ap.add_argument('--no-sequence-pass', action='store_true', help='skip the extra (untimed-for-the-metric) pass in the reference\'s default stage order')
    ap.add_argument('--inflight', type=int, default=6, help='frames in flight per GPU (worker streams); 1 = strictly sequential')
    args = ap.parse_args()
    if args.steps < 1 or args.blocks < 1 or args.steps % args.blocks:
        ap.error(f'--steps ({args.steps}) must be a positive multiple of --blocks ({args.blocks})')

    import faulthandler
    faulthandler.enable()
    if int(os.environ.get('VG_BENCH_WATCHDOG', 0)) > 0:           # development aid: dump every thread's stack and exit if the run stalls
        faulthandler.dump_traceback_later(int(os.environ['VG_BENCH_WATCHDOG']), exit=True)
    world = int(os.environ.get('WORLD_SIZE', 1))
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    if world != args.gpus:
        sys.exit(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus} '
                 f'(or run `python bench.py --gpus {args.gpus}` without a launcher)')
    import torch
    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        backend = os.environ.get('VILGOD_DIST_BACKEND', 'nccl')       # 'gloo' only for the 2-ranks-on-one-GPU self test
        kw = {'device_id': torch.device(f'cuda:{local_rank}')} if backend == 'nccl' else {}
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    dev = torch.device(f'cuda:{local_rank}')
    torch.cuda.set_device(dev)

    from vilgod_amd import synthetic, dist as vdist
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pipe = PseudoLabelPipeline(device=dev, vit_dtype=args.dtype, n_views=args.views, max_points=args.points + 1024,
                               clip_model_path='/nonexistent', box_mode=args.box_mode, vit_graph=args.vit_graph, angle_mode=args.angle_mode)
    B = args.blocks                                  # timed blocks (each exactly K steps, each on its own distinct clouds)
    K, W = args.steps // B, max(args.warmup, args.inflight if args.inflight > 1 else 0)       # warm-up covers the worker handles
    # ONE sequence of world * K timed frames (+ a warm-up stretch in front), contiguous block of K frames per rank, smooth
    # trajectory; every frame of the stream is a distinct seeded cloud (pinned host memory; `--input resident`: in HBM)
    poses = synthetic.make_poses(W + world * K + 8, seed=0)
    host_frames = [torch.from_numpy(synthetic.make_frame(1 + rank * 100_000 + i, args.points, n_objects=args.objects)).pin_memory()
                   for i in range(W + B * K)]
    frames = [f.to(dev) for f in host_frames] if args.input == 'resident' else host_frames
    if args.input == 'host':
        # a block's input copies are all queued up front, one device buffer per frame: bring torch's caching allocator to the
        # steady state of a long-running stream (later blocks recycle the buffers of earlier ones) instead of K fresh,
        # device-synchronising hipMalloc calls inside the first timed block.  Not a step: no frame is processed here.
        prime = [torch.empty_like(host_frames[0], device=dev) for _ in range(K)]
        del prime
    torch.cuda.synchronize()
    inflight = 1 if args.stage_times else max(1, args.inflight)
    stage = {}

    def run_steps(p, first_pose, count, first_fnr, after_ground=None, first_frame=0, src=None):
        """`count` frames whose poses start at index `first_pose` and whose clouds start at `first_frame` of the stream;
        returns [(FrameState, result, probs)]."""
        src = frames if src is None else src
        idx = list(range(count))
        if inflight == 1:
            out = []
            for i in idx:
                fs, res = p.process_frame(p.upload(src[first_frame + i]), poses[first_pose + i], poses[0], fnr=first_fnr + i, timing=args.stage_times)
                out.append((fs, res, p.last_probs))
                for k, v in p.timings.items():
                    stage[k] = stage.get(k, 0.0) + v
            if after_ground is not None:
                after_ground()
            return out
        return p.process_frames([src[first_frame + i] for i in idx], [poses[first_pose + i] for i in idx], poses[0],
                                n_workers=inflight, first_fnr=first_fnr, after_ground=after_ground)

    def timed_block(p, b=0):
        """The timed region of one rank: ground-state hand-off + K frames + the one all-gather.  -> (elapsed, outputs).
        b: which block of K distinct clouds of the stream (frames[W + b K : W + (b + 1) K])."""
        off = W + b * K
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.new_sequence()
        out = []
        if world > 1 and args.ground_handoff == 'relay':
            # frames dealt round-robin as in `replicate`, but every rank runs ONLY its own ground passes: the Patchwork++ state is relayed
            # frame by frame (rank g % N takes it from rank (g - 1) % N before frame g, hands it on behind it; vilgod_amd/dist.py)
            seq = [frames[off + g // world] for g in range(world * K)]
            seq_poses = [poses[W + g] for g in range(world * K)]
            mine = [g for g in range(world * K) if g % world == rank]
            rl = (lambda g: vdist.relay_recv_state(p.ground_model, g, dev), lambda g: vdist.relay_send_state(p.ground_model, g, world * K, dev))
            if inflight == 1:
                for g in mine:
                    rl[0](g)
                    d_pts = p.upload(seq[g])
                    mask_g = p.ground(d_pts)
                    rl[1](g)                      # the state goes on before this frame's heavy stages start
                    fs, res = p.process_frame(d_pts, seq_poses[g], poses[0], fnr=g, timing=args.stage_times, mask=mask_g)
                    out.append((fs, res, p.last_probs))
            else:
                out = p.process_frames(seq, seq_poses, poses[0], n_workers=inflight, first_fnr=0, own=mine, relay=rl)
        elif world > 1 and args.ground_handoff == 'replicate':
            # frames dealt round-robin: frame g of the N * K frame sequence belongs to rank g % N.  Every rank queues the upload + ground
            # pass of ALL frames, in order, on its high-priority ground stream (0.36 ms per scan: N * K passes against K * ~15 ms of own
            # work) and processes its own frames in full; rank r's first frame waits for r ground passes, no state is exchanged.
            # (The other ranks' clouds are not held here: this rank's own stand in, same upload and ground cost.)
            seq = [frames[off + g // world] for g in range(world * K)]
            seq_poses = [poses[W + g] for g in range(world * K)]
            mine = [g for g in range(world * K) if g % world == rank]
            if inflight == 1:
                for g in range(world * K):
                    d_pts = p.upload(seq[g])
                    if g % world == rank:
                        fs, res = p.process_frame(d_pts, seq_poses[g], poses[0], fnr=g, timing=args.stage_times)
                        out.append((fs, res, p.last_probs))
                    else:
                        p.ground(d_pts)
            else:
                out = p.process_frames(seq, seq_poses, poses[0], n_workers=inflight, first_fnr=0, own=mine)
        elif world > 1 and args.ground_handoff == 'replay':
            for i in range(rank * K):                    # the frames before this rank's block: ground stage only (the other ranks'
                p.ground(p.upload(frames[off + i % K]))  # clouds are not held here: this rank's own stand in, same cost)
            out = run_steps(p, W + rank * K, K, rank * K, first_frame=off)
        elif world > 1:
            # chain: the block's ground passes are queued first on the caller's stream (process_frames does that), the state after
            # them is exported and sent on while the workers are already busy with the block's frames
            vdist.recv_ground_state(p.ground_model, dev)
            out = run_steps(p, W + rank * K, K, rank * K, after_ground=lambda: vdist.send_ground_state(p.ground_model, dev), first_frame=off)
        else:
            out = run_steps(p, W, K, 0, first_frame=off)
        score_mats = [probs for _, _, probs in out]
        # the one collective of the path: all-gather of the per-crop score matrices (padded to a common length)
        scores = torch.cat(score_mats) if score_mats else torch.zeros((0, 24), device=dev)
        if dist is not None:
            cdev = 'cpu' if dist.get_backend() == 'gloo' else dev
            n_loc = torch.tensor([scores.shape[0]], device=cdev, dtype=torch.int64)
            n_all = [torch.zeros_like(n_loc) for _ in range(world)]
            dist.all_gather(n_all, n_loc)
            mx = int(max(int(x.item()) for x in n_all))
            pad = torch.zeros((mx, scores.shape[1]), device=dev, dtype=scores.dtype)
            pad[:scores.shape[0]] = scores
            gathered = torch.empty((world * mx, scores.shape[1]), device=dev, dtype=scores.dtype)
            if dist.get_backend() == 'gloo':                  # host-staged in the self test; RCCL gathers device tensors directly
                parts = [torch.empty_like(pad.cpu()) for _ in range(world)]
                dist.all_gather(parts, pad.cpu())
                gathered = torch.cat(parts).to(dev)
            else:
                dist.all_gather_into_tensor(gathered, pad)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        t = torch.tensor([elapsed], device='cpu' if (dist is not None and dist.get_backend() == 'gloo') else dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), out

    def comm_warmup():
        """Every communication path of the timed region once before it (RCCL builds its point-to-point and collective
        communicators lazily, seconds on first use): the state hand-off down the rank chain, the two all-gathers, the all-reduce."""
        if dist is None:
            return
        from vilgod_amd._lib import lib as _l
        cdev = 'cpu' if dist.get_backend() == 'gloo' else dev
        if args.ground_handoff == 'chain':               # (replicate / replay exchange no state: no point-to-point communicator is built)
            buf = torch.zeros(int(_l.vg_ground_state_bytes()), dtype=torch.uint8, device=cdev)
            if rank > 0:
                dist.recv(buf, src=rank - 1)
            if rank < world - 1:
                dist.send(buf, dst=rank + 1)
        if args.ground_handoff == 'relay':               # the ring rank -> rank + 1 (-> 0): the same order of operations as the timed region's first round
            buf = torch.zeros(int(_l.vg_ground_state_bytes()), dtype=torch.uint8, device=cdev)
            if rank > 0:
                dist.recv(buf, src=rank - 1)
            dist.send(buf, dst=(rank + 1) % world)
            if rank == 0:
                dist.recv(buf, src=world - 1)
        one = torch.ones(1, dtype=torch.int64, device=cdev)
        dist.all_gather([torch.zeros_like(one) for _ in range(world)], one)
        if dist.get_backend() != 'gloo':
            dist.all_gather_into_tensor(torch.empty((world * 8, 24), device=dev), torch.zeros((8, 24), device=dev))
        else:
            dist.all_gather([torch.zeros(8, 24) for _ in range(world)], torch.zeros(8, 24))
        dist.all_reduce(torch.zeros(1, dtype=torch.float64, device=cdev), op=dist.ReduceOp.MAX)
        torch.cuda.synchronize()
        dist.barrier()

    pipe.new_sequence()
    # Set-up before the warm-up (not steps of the metric; distinct clouds of their own): one block of the timed block's length
    # brings torch's caching allocator to the steady state of a long-running stream.  Every frame in flight allocates its
    # temporaries (non-ground points, packed clusters, crops' patch rows, ViT workspace ...) through it, and the first block of a
    # process that needs a new size pays a device-synchronising hipMalloc inside the timed region: measured on K = 20, the metric's
    # block -- the first of the process -- read 55.4 frames/s while every later block of the same run (same frames, other pipeline
    # objects) read 57.8-59.2.  Model set-up like weight loading; reported as config.setup_frames.
    # The block is repeated until two consecutive passes take the same time within 3 % (at least 3, at most 8 passes): the first process on a
    # freshly leased box runs its first 0.6-1.5 s of GPU work 2-4x slower than everything after it (measured: set-up passes of 575,
    # 322, 325, 321 ms on such a box; with a single pass the timed block of a first process read 42-44 frames/s, the second process
    # on the same box 54-60) -- a property of the box's first load, not of the steady stream the metric describes.
    n_setup = 0 if args.stage_times else min(K, 24)
    setup_passes = 0
    setup_frames = []
    if n_setup:
        setup_frames = [torch.from_numpy(synthetic.make_frame(900_001 + rank * 100_000 + i, args.points, n_objects=args.objects)).pin_memory()
                        for i in range(n_setup)]
        last = None
        while setup_passes < 8:
            torch.cuda.synchronize()
            t_s = time.perf_counter()
            run_steps(pipe, 0, n_setup, 0, src=setup_frames)
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t_s
            pipe.new_sequence()
            setup_passes += 1
            # (round 5: at least three passes and 3 % instead of two and 5 %.  It does not change what the timed blocks read -- their spread,
            # 63.5 / 67 / 68.5 frames/s at K = 20, is the blocks' DATA: 337.6 / 328.4 / 323.6 crops per frame, `block_crops_per_frame`)
            if setup_passes >= 3 and last is not None and abs(dt_s - last) <= 0.03 * last:
                break
            last = dt_s
    run_steps(pipe, 0, W, 0)                                   # warm-up, also builds the worker handles
    comm_warmup()
    stage = {}
    def graph_stats(p):
        st = [w._graph_cls.stats() for w in (p._workers or []) + [p] if getattr(w, '_graph_cls', None) is not None]
        return {k: sum(s_[k] for s_ in st) for k in ('graphs_captured', 'graph_launches', 'graphs_evicted', 'graphs_live')} if st else \
            {'graphs_captured': 0, 'graph_launches': 0, 'graphs_evicted': 0, 'graphs_live': 0}

    g_before = graph_stats(pipe)
    # B blocks of EXACTLY K steps each, every block on its own K distinct clouds and bracketed by its own barrier + synchronize (timed_block);
    # the reported block is the MEDIAN one (its elapsed time, its outputs): a single 0.3 s window decided round 4's number to +-4 %
    blocks_run = [timed_block(pipe, b) for b in range(B)]
    order = sorted(range(B), key=lambda b: blocks_run[b][0])
    elapsed, outs = blocks_run[order[(B - 1) // 2]]
    block_elapsed = [e for e, _ in blocks_run]
    outs0 = blocks_run[0][1]                         # block 0 = frames[W : W + K]: the frames the information blocks below process again
    if args.dump_outputs and rank == 0 and blocks_run[-1][1]:
        dump_outputs(args.dump_outputs, blocks_run[-1][1][-1], pipe.mapped_names)       # the last timed step of this rank
    g_after = graph_stats(pipe)
    crops = sum(p.shape[0] for _, _, p in outs)
    clusters = sum(fs.n_detections for fs, _, _ in outs)
    labelled = sum(len(res['name']) for _, res, _ in outs)

    # roofline of the dominant kernel: HIP event pairs around every launch of it on its launch stream, over a SEQUENTIAL pass
    # (1 frame in flight) of the same workload right after the timed region -- with several frames in flight the pairs would
    # also span other streams' kernels and stop measuring this kernel.
    launches = gemm_ms = gemm_flops = all_launches = all_ms = all_flops = 0
    # the FIRST six clouds of the stream: the frames tools/collect_profiles.sh's run (--warmup 2 --steps 4 --inflight 1) processes, so
    # that the live average and the rocprofv3 kernel-trace average are taken over the same launches (the average launch time follows
    # the frame's crop count)
    n_pass = min(6, W + K)
    roofline_pass = args.full and not args.no_roofline_pass
    if roofline_pass:
        pipe.clip.encoder.profile(True)
        for i in range(n_pass):
            pipe.process_frame(pipe.upload(frames[i]), poses[i + 1], poses[0], fnr=i)
        launches, gemm_ms, gemm_flops = pipe.clip.encoder.profile_read(kind=1)        # the dominant kernel alone
        all_launches, all_ms, all_flops = pipe.clip.encoder.profile_read(kind=-1)
        pipe.clip.encoder.profile(False)

    # Latency of ONE frame on the otherwise idle GPU, stage by stage (pipeline.process_frame(timing=True): a device synchronisation behind
    # every stage; medians over six frames after two untimed ones).  Not a throughput figure: it is what an online user waits for, and what a
    # timed block pays once while its pipeline fills (the first frame's front stage runs on an empty GPU before the first GEMM starts).
    frame_latency = None
    if roofline_pass and not args.stage_times and world == 1:
        rows_l = []
        pipe.new_sequence()
        for i in range(min(8, W + K)):
            torch.cuda.synchronize()
            pipe.process_frame(frames[i], poses[i + 1], poses[0], fnr=i, timing=True)
            if i >= 2:
                rows_l.append(dict(pipe.latency))
        if rows_l:
            med_l = {k: round(1e3 * float(np.median([r.get(k, 0.0) for r in rows_l])), 3) for k in rows_l[0]}
            back_keys = ('encode+scores', 'scores_d2h+box_wait', 'vote+results')
            frame_latency = dict(med_l, total=round(sum(med_l.values()), 3),
                                 front_stage_until_the_crops_are_queued=round(sum(v for k, v in med_l.items() if k not in back_keys), 3),
                                 note='one frame at a time on an idle GPU, a device synchronisation behind every stage (sum = the frame\'s latency; '
                                      'inside the stream the stages of different frames overlap)')

    # The tower the way the pipeline runs it: TWO encodes in flight (pipeline._vit_in_turn), every kernel of the tower counted.  The
    # sequential pass above times one launch at a time and so pays, per launch, for the partial last round of 256 x 256 tiles (333 crops
    # are 257 row tiles x 3 column tiles = 3.01 rounds of 256 CUs for out_proj / c_proj); two encodes in flight fill each other's tails,
    # which is what the timed region sees (tools/exp_tile_tail.py: 40.4 us per crop whatever the crop count, against 42-46 with one).
    tower2 = None
    if roofline_pass and not args.stage_times and args.dtype == 'f16':
        import threading
        n_cr = int(round(sum(p_.shape[0] for _, _, p_ in outs) / max(len(outs), 1))) or 337
        rows2 = (n_cr * 196 + 255) // 256 * 256
        views2 = [pipe.clip.encoder.view(), pipe.clip.encoder.view()]
        streams2 = [torch.cuda.Stream(device=dev) for _ in range(2)]
        pat2 = [(torch.randint(0, 256, (rows2, 256), device=dev).float() / 256).half() for _ in range(2)]
        reps2 = 8

        def loop2(k, reps):
            with torch.cuda.stream(streams2[k]):
                for _ in range(reps):
                    views2[k].encode_patches(pat2[k], n_cr)
                streams2[k].synchronize()
        for k in range(2):
            loop2(k, 2)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        th2 = [threading.Thread(target=loop2, args=(k, reps2)) for k in range(2)]
        [t.start() for t in th2]
        [t.join() for t in th2]
        torch.cuda.synchronize()
        t2 = (time.perf_counter() - t2) / (2 * reps2)
        tower2 = {'crops': n_cr, 'ms_per_encode': round(1000.0 * t2, 3), 'us_per_crop': round(1e6 * t2 / n_cr, 2),
                  'achieved': round(VIT_FLOP_PER_CROP * n_cr / t2 / 1e12, 1), 'unit': 'TFLOP/s',
                  'frac': round(VIT_FLOP_PER_CROP * n_cr / t2 / 1e12 / PEAK_F16_MFMA_TFLOPS, 4),
                  'note': 'the whole ViT-B/16 tower (projection GEMMs, attention, embedding, head: 35.1 GFLOP per crop, SURVEY 8d) on random '
                          'single-channel patch rows of the stream\'s mean crop count, two encodes in flight on two streams (the pipeline lets up to three ViT passes run at a time since round 6: VILGOD_VIT_CONCURRENCY); wall '
                          'time per encode.  Not the kernel roofline (that is `frac` above, one launch at a time): what the timed region gets'}
        del views2, pat2

    if rank == 0:
        frames_total = world * K
        value = frames_total / elapsed
        achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        traffic = traffic_src = by_kind = pmc_mfma = None
        tpath = os.path.join(ROOT, 'profiles', 'gemm_traffic.json')       # tools/collect_profiles.sh + summarize_profiles.py
        if args.full and os.path.exists(tpath):
            tj = json.load(open(tpath))
            traffic = round(tj['hbm_bytes_per_launch'])
            by_kind, pmc_mfma = tj.get('by_kind') or None, tj.get('mfma_utilisation')
            traffic_src = f"profiles/gemm_traffic.json ({tj.get('kernel', '?')}, {tj.get('tag', '?')}): rocprofv3 PMC passes of this command, not measured in this run"
        out = {
            'metric': 'pseudo-labeled LiDAR frames/sec (150k pts, ~60 clusters)',
            'value': round(value, 3), 'unit': 'frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'blocks': B, 'block_values': [round(frames_total / e, 3) for e in block_elapsed],
            'block_spread': round((max(block_elapsed) - min(block_elapsed)) / elapsed, 4),
            'block_crops_per_frame': [round(sum(p_.shape[0] for _, _, p_ in o) / max(len(o), 1), 1) for _, o in blocks_run],      # the blocks' clouds differ: ms per frame follows the crop count
            'ms_per_step': round(1000.0 * elapsed / K, 3), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f16' if args.dtype == 'f16' else 'f32', 'data': 'synthetic',
            'config': {
                'workload': (f'full per-frame path (ground removal, HDBSCAN, filters, {args.views}-view render, CLIP ViT-B/16 '
                             f'{args.dtype} encode, scores, vote, boxes [{args.box_mode} mode]) on synthetic {args.points}-pt frames, '
                             f'{args.objects} objects (BASELINE config 3 shape' + (' as written' if args.views == 6 else f', but {args.views} views as in the reference\'s waymo.yaml; the 6-view '
                             'form is the views6 block') + f'), ONE sequence of {frames_total} frames sharded '
                             f'{world}-way ' + (('round-robin, ground pass replicated on every rank (no state exchange)' if args.ground_handoff == 'replicate'
                                                else 'round-robin, ground state relayed frame by frame (every rank runs its own ground passes only)' if args.ground_handoff == 'relay'
                                                else f'in contiguous blocks, ground state by {args.ground_handoff}') if world > 1 else '(one rank)') +
                             ', one all-gather of the score matrices'),
                'points_per_frame': args.points, 'views': args.views, 'frames_per_gpu': K,
                'setup_frames': n_setup * setup_passes,
                'distinct_frames': len({id(f) for f in frames[W:W + B * K]}), 'distinct_crop_counts': len({int(p.shape[0]) for _, _, p in outs}),
                'input': ('pinned host buffers, H2D copy inside the timed region' if args.input == 'host' else 'resident in HBM before the timed region'),
                'vit_launch': 'captured hipGraphs per crop-count bucket' if args.vit_graph else 'plain stream launches',
                'value_is': (f'one timed block of {K} steps' if B == 1 else
                             f'the median of {B} timed blocks of {K} steps each (block_values; the --steps frames split into blocks of equal length on their own distinct clouds, own barrier + synchronize brackets)'),
                'graphs_captured': g_after['graphs_captured'] - g_before['graphs_captured'],
                'graph_launches': g_after['graph_launches'] - g_before['graph_launches'],
                'angle_mode': args.angle_mode,
                'clusters_per_frame': round(clusters / max(K, 1), 1),
                'nonground_points_per_frame': round(sum(int(getattr(fs, 'n_nonground', 0) or 0) for fs, _, _ in outs) / max(K, 1)),
                'crops_per_frame': round(crops / max(K, 1), 1),
                'labelled_per_frame': round(labelled / max(K, 1), 1),
                'weights': pipe.clip.weights_source, 'parallelism': f'frame-sharded x{world}', 'frames_in_flight_per_gpu': inflight, 'vit_passes_at_a_time': int(os.environ.get('VILGOD_VIT_CONCURRENCY', '3')),
                'box_mode': args.box_mode,
            },
        }
        if args.full:
            out['roofline'] = {
                'kernel': f'{DOMINANT_KERNEL} (every ViT projection GEMM: in_proj, out_proj, c_fc, c_proj, patch embedding)',
                'bound': 'mfma', 'achieved': round(achieved, 1), 'peak': PEAK_F16_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                'frac': round(achieved / PEAK_F16_MFMA_TFLOPS, 4), 'traffic': traffic, 'traffic_unit': 'HBM bytes per launch (PMC)',
                'traffic_source': traffic_src,
                'method': f'HIP event pairs on the launch stream around every {DOMINANT_KERNEL} launch, sequential pass (1 frame in flight) over the first {n_pass} clouds of the stream right after the timed region (the frames of the committed rocprofv3 run)',
                'note': 'the launches also carry the blocks\' LayerNorms (folded into the GEMM epilogues; their work is not counted in the algorithmic FLOPs). '
                        'Like for like: with separate LayerNorm kernels (VG_VIT_LN_FOLD=0) the GEMM launches alone reach 0.31, GEMM + LayerNorm launches together 0.29 '
                        '(13.96 + 1.27 ms per frame against 14.67 ms now, profiles/r02i vs r02l)',
                'launches': launches, 'avg_launch_us': round(1000.0 * gemm_ms / max(launches, 1), 2),
                'algorithmic_flops_per_launch': round(gemm_flops / max(launches, 1)),
                'gemm_ms_per_frame': round(gemm_ms / max(n_pass, 1), 3),
                'tower_two_in_flight': tower2,
                'mfma_utilisation_pmc': pmc_mfma,
                'by_kind_pmc': by_kind,      # per GEMM kind of the full-size blocks: time, FETCH / WRITE against algorithmic bytes, MFMA busy (the same PMC passes as `traffic`)
                'all_projection_gemms': {'launches': all_launches,
                                         'achieved': round(all_flops / (all_ms * 1e-3) / 1e12, 1) if all_ms > 0 else 0.0,
                                         'ms_per_frame': round(all_ms / max(n_pass, 1), 3)},
            }
        # scalars inside `config` / `roofline` (a record that keeps only scalar keys of those two still carries the evidence; VERDICT r5 task 5)
        bvals, bcrops = out['block_values'], out['block_crops_per_frame']
        for i, (bv, bc) in enumerate(zip(bvals, bcrops)):
            out['config'][f'block{i}_value'] = bv
            out['config'][f'block{i}_crops'] = bc
        out['config']['us_per_crop'] = round(1e6 * elapsed / max(crops, 1), 2)
        out['config']['gemm_kernel'] = DOMINANT_KERNEL
        out['config']['hierarchy_stage'] = pipe.hierarchy        # HDBSCAN's hierarchy stage: 'device' (csrc/hdbscan_device.hip) or 'host'
        out['value_block0'] = bvals[0]                 # the clouds rounds 1-4 timed as their single block: comparable across rounds
        if tower2 is not None:
            out['roofline']['tower2_frac'] = tower2['frac']
            out['roofline']['tower2_us_per_crop'] = tower2['us_per_crop']
        if by_kind and by_kind.get('out_proj', {}).get('hbm_tb_per_s') is not None:
            out['roofline']['out_proj_tb_per_s'] = by_kind['out_proj']['hbm_tb_per_s']
        if frame_latency is not None:
            out['frame_latency_ms'] = frame_latency
            out['roofline']['front_stage_latency_ms'] = frame_latency['front_stage_until_the_crops_are_queued']
        if args.stage_times:
            out['stage_ms_per_frame'] = {k: round(1000.0 * v / K, 3) for k, v in stage.items()}
        if args.full and world == 1 and not args.stage_times and not args.no_extras:
            def multi_gpu_model():
                # what frame sharding costs, from this GPU's own numbers (no multi-GPU node is available to the builder; the driver's
                # SCALE file is the measurement): t_f = this run's ms per step, t_g = a ground pass (upload + kernels) timed back to back in
                # the steady state of its adaptive stores.  chain (contiguous blocks, state handed down): rank r starts r*K*t_g late ->
                # efficiency t_f / (t_f + (N-1) t_g) whatever K.  replicate (round-robin, every rank runs all passes): the first frame of
                # rank r waits r*t_g and every rank spends N*t_g of ground-stream time per own frame, under its ViT work when
                # N*t_g < t_f -> K*t_f / (K*t_f + (N-1) t_g).
                pipe.new_sequence()
                fr = [pipe.upload(f) for f in host_frames[:min(8, len(host_frames))]]
                for _ in range(6):
                    for f in fr:
                        pipe.ground(f)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for _ in range(5):
                    for f in fr:
                        pipe.ground(pipe.upload(host_frames[n % len(fr)]) if args.input == 'host' else f)
                        n += 1
                torch.cuda.synchronize()
                t_g = 1000.0 * (time.perf_counter() - t0) / n
                t_f = 1000.0 * elapsed / K

                # MEASURED on this one GPU (VERDICT r5 task 2): what rank 0 of N pays.  The process runs exactly what rank 0 of the
                # replicated round-robin design runs -- process_frames over the N K frame sequence with own = every N-th frame: all N K
                # uploads + ground passes on the ground stream, K own frames in full -- against the plain K-frame block on the SAME clouds,
                # the two interleaved, median of three.  (A rank r > 0 does the same work; its first frame waits r passes longer.)  The
                # chain design's rank N - 1 is its K own frames behind the (N - 1) K ground passes of the ranks before it (the recv it
                # waits for), timed here as that many ground passes on an otherwise idle GPU plus the plain block.
                def one_block(N, off):
                    seq = [frames[off + g // N] for g in range(N * K)]
                    seq_poses = [poses[W + (g % (world * K))] for g in range(N * K)]
                    mine = [g for g in range(N * K) if g % N == 0]
                    torch.cuda.synchronize()
                    t0_ = time.perf_counter()
                    pipe.new_sequence()
                    if N == 1:
                        pipe.process_frames(seq, seq_poses, poses[0], n_workers=inflight, first_fnr=0)
                    else:
                        pipe.process_frames(seq, seq_poses, poses[0], n_workers=inflight, first_fnr=0, own=mine)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0_
                emu = {}
                worlds = [int(n_) for n_ in (args.emulate_world or []) if int(n_) > 1]
                if worlds and inflight > 1:
                    off_e = W                                   # block 0's clouds
                    for n_ in [1] + worlds:
                        one_block(n_, off_e)                    # untimed pass per shape (the own = ... path's first use)
                    times = {n_: [] for n_ in [1] + worlds}
                    for _ in range(3):
                        for n_ in [1] + worlds:
                            times[n_].append(one_block(n_, off_e))
                    med = {n_: float(np.median(v)) for n_, v in times.items()}
                    for n_ in worlds:
                        chain_wait = (n_ - 1) * K * t_g * 1e-3
                        emu[str(n_)] = {'own_frames_per_s': round(K / med[n_], 3), 'plain_frames_per_s': round(K / med[1], 3),
                                        'replicate_efficiency_measured': round(med[1] / med[n_], 4),
                                        'replicate_efficiency_modelled': round(K * t_f / (K * t_f + (n_ - 1) * t_g), 4),
                                        'chain_last_rank_efficiency': round(med[1] / (med[1] + chain_wait), 4)}
                return {'t_frame_ms': round(t_f, 3), 't_ground_pass_ms': round(t_g, 3), 'frames_per_gpu': K,
                        'measured_single_rank_emulation': emu or None,
                        'measured_how': ('rank 0 of N on this one GPU: process_frames(N K frames, own = every N-th) against the plain K-frame block on the '
                                         'same clouds (block 0), interleaved, median of 3; chain: (N - 1) K ground passes at the measured t_ground_pass_ms '
                                         'in front of the plain block.  What it cannot show: RCCL (one all-gather of ~0.6 MB of scores per block) and '
                                         'PCIe / host contention between eight ranks of one node'),
                        'weak_scaling_efficiency_modelled': {
                            str(N): {'replicate_round_robin': round(K * t_f / (K * t_f + (N - 1) * t_g), 4),
                                     'chain_blocks': round(t_f / (t_f + (N - 1) * t_g), 4),
                                     'ground_stream_share_of_a_frame': round(N * t_g / t_f, 3)} for N in (2, 4, 8)},
                        'note': 'modelled = a prediction from t_frame and t_ground (assumes the replicated passes are free under the ViT work); '
                                'measured_single_rank_emulation = the same design run by one rank on this GPU; bench.py --gpus N on a multi-GPU node '
                                'measures the rest (SCALE file; no such node was available to the builder: no RCCL run exists)'}
            block_early = multi_gpu_model
            try:
                out['multi_gpu_model'] = block_early()
            except Exception as e:          # noqa: BLE001
                out['multi_gpu_model'] = {'error': f'{type(e).__name__}: {e}'}
            for n_, rec in ((out['multi_gpu_model'].get('measured_single_rank_emulation') or {}).items()):
                out['config'][f'rank0_of_{n_}_efficiency_measured'] = rec['replicate_efficiency_measured']      # (scalar copies, see above)
        extras = args.full and world == 1 and not args.no_extras and not args.stage_times

        def block(name, fn):
            """An information block must never cost the metric line: failures are reported inside the JSON."""
            try:
                t0 = time.perf_counter()
                out[name] = fn()
                if isinstance(out[name], dict):
                    out[name]['block_seconds'] = round(time.perf_counter() - t0, 1)
            except Exception as e:          # noqa: BLE001
                out[name] = {'error': f'{type(e).__name__}: {e}'}

        def settle(p2, points, objects):
            """The metric's untimed set-up for an information block's fresh pipeline object (only the headline had it, so
            the blocks read 20-30 % low and their A/B pairs were confounded): blocks of distinct clouds -- the metric's own set-up clouds
            for its shape, 24 new ones otherwise -- until two consecutive passes agree within 5 % (at most 5): worker handles, ViT
            workspaces and the caching allocator reach the state of a long-running stream before the block's clock starts."""
            if points == args.points and objects == args.objects and setup_frames:
                sf = setup_frames
            else:
                sf = [torch.from_numpy(synthetic.make_frame(700_001 + i, points, n_objects=objects)).pin_memory() for i in range(min(K, 24))]
            last = None
            for _ in range(5):
                p2.new_sequence()
                torch.cuda.synchronize()
                t_s = time.perf_counter()
                p2.process_frames(sf, [poses[i] for i in range(len(sf))], poses[0], n_workers=inflight)
                torch.cuda.synchronize()
                dt_s = time.perf_counter() - t_s
                if last is not None and abs(dt_s - last) <= 0.05 * last:
                    break
                last = dt_s

        def other_shape(points, objects, views, steps, box_mode=None, vit_graph=None, resident=None, angle_mode=None):
            """The metric's run on a second pipeline object (same tower) with one knob changed, or on another frame shape: `steps`
            distinct clouds after a warm-up stretch of distinct clouds, same input mode as the metric unless `resident` says otherwise."""
            p2 = PseudoLabelPipeline(device=dev, vit_dtype=args.dtype, n_views=views, max_points=points + 1024, clip_model_path='/nonexistent',
                                     clip=pipe.clip, box_mode=box_mode or args.box_mode,
                                     vit_graph=args.vit_graph if vit_graph is None else vit_graph, angle_mode=angle_mode or args.angle_mode)
            if points == args.points and objects == args.objects:
                fr = host_frames
            else:
                fr = [torch.from_numpy(synthetic.make_frame(501 + i, points, n_objects=objects)).pin_memory() for i in range(W + steps)]
            if (args.input == 'resident') if resident is None else resident:
                fr = [f.to(dev) for f in fr]
            settle(p2, points, objects)
            p2.new_sequence()
            p2.process_frames(fr[:W], [poses[i] for i in range(W)], poses[0], n_workers=inflight)      # warm-up: worker handles
            p2.new_sequence()
            torch.cuda.synchronize()
            g0 = graph_stats(p2)
            t0 = time.perf_counter()
            res = p2.process_frames(fr[W:W + steps], [poses[W + i] for i in range(steps)], poses[0], n_workers=inflight)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            other_shape.graphs = {k: v - g0[k] for k, v in graph_stats(p2).items()}
            # this block's pipeline (six workers' cluster / ViT handles: gigabytes of device buffers) is released HERE, outside any
            # timed region: left to the garbage collector its hipFree calls (device-synchronising) landed inside a later block's clock
            p2._workers = None
            del p2, fr
            import gc
            gc.collect()
            torch.cuda.synchronize()
            return dt, res

        if extras:
            def box_modes():
                other = 'fast' if args.box_mode == 'reference' else 'reference'
                dt, res = other_shape(args.points, args.objects, args.views, K, box_mode=other)
                n = differ = 0
                for (fa, _, _), (fb, _, _) in zip(outs0, res):
                    if fa.boxes is None or fb.boxes is None:
                        continue
                    rows = np.flatnonzero(fa.valid)
                    a, b = fa.boxes[rows], fb.boxes[rows]
                    n += len(rows)
                    differ += int((np.abs(a[:, 3] * a[:, 4] - b[:, 3] * b[:, 4]) > 2e-4 * np.maximum(1.0, a[:, 3] * a[:, 4])).sum())
                return {args.box_mode: {'value': round(value, 3), 'unit': 'frames/s'}, other: {'value': round(K / dt, 3), 'unit': 'frames/s'},
                        'boxes_compared': n, 'boxes_that_differ': differ,
                        'note': "same frames, same steps; 'reference' = the reference's boxes (qhull vertex order, closing hull edge dropped: "
                                "host qhull on the worker threads), 'fast' = GPU hull + rectangle over all edges; a box differs when its "
                                'footprint area differs by more than 2e-4 relative'}
            block('box_modes', box_modes)

            def hipgraph_loop():
                on = args.vit_graph
                dt, res = other_shape(args.points, args.objects, args.views, K, vit_graph=not on)
                same = all(np.array_equal(a[1]['name'], b[1]['name']) and np.array_equal(a[2].cpu().numpy(), b[2].cpu().numpy()) for a, b in zip(outs0, res))
                gs = other_shape.graphs if not on else {k: g_after[k] - g_before[k] for k in g_after}
                return {'captured': {'value': round(value if on else K / dt, 3), 'unit': 'frames/s'},
                        'plain_launches': {'value': round(K / dt if on else value, 3), 'unit': 'frames/s'},
                        'identical_scores_and_names': bool(same),
                        'graphs_captured_in_timed_region': gs['graphs_captured'], 'graph_launches': gs['graph_launches'],
                        'graphs_evicted': gs['graphs_evicted'], 'distinct_crop_counts': len({int(r[2].shape[0]) for r in res}),
                        'note': 'captured = the ViT encode + scores of a frame (~150 kernels) replayed as one hipGraph per crop-count bucket (crops '
                                'rounded up to a multiple of 8, padding crops never read), per worker, at most 32 graphs kept (LRU); the captures of '
                                'this distinct-frame stream happen inside the timed region.  Ground / clustering / rendering have frame-dependent '
                                'launch dimensions and the hierarchy is built on the host, so they stay stream launches around the graph (BASELINE config 5)'}
            block('hipgraph_loop', hipgraph_loop)

            def shape_block(points, objects, views, cfg_name):
                def fn():
                    dt, res = other_shape(points, objects, views, K)
                    return {'value': round(K / dt, 3), 'unit': 'frames/s', 'steps': K, 'points_per_frame': points, 'objects': objects, 'views': views,
                            'clusters_per_frame': round(sum(r[0].n_detections for r in res) / K, 1),
                            'crops_per_frame': round(sum(r[2].shape[0] for r in res) / K, 1), 'workload': cfg_name}
                return fn
            def resident_input():
                dt, res = other_shape(args.points, args.objects, args.views, K, resident=(args.input == 'host'))
                same = all(np.array_equal(a[1]['name'], b[1]['name']) for a, b in zip(outs0, res))
                return {'value': round(K / dt, 3), 'unit': 'frames/s', 'bytes_per_frame': int(host_frames[0].numel() * host_frames[0].element_size()),
                        'same_names_as_metric_run': bool(same),
                        'note': ('the same steps with every frame uploaded to HBM before the clock starts' if args.input == 'host' else
                                 'the same steps with every frame handed over as a pinned HOST buffer (the copy to HBM inside the timed region)')}
            block('resident_input' if args.input == 'host' else 'host_input', resident_input)

            def angle_modes():
                other = 'reference' if args.angle_mode == 'device' else 'device'
                dt, res = other_shape(args.points, args.objects, args.views, K, angle_mode=other)
                n = flips = 0
                for a, b in zip(outs0, res):
                    if np.array_equal(a[0].valid, b[0].valid) and pipe.cls_key in a[0].cls and pipe.cls_key in b[0].cls:
                        rows = np.flatnonzero(a[0].valid)
                        n += len(rows)
                        flips += int(sum(str(a[0].cls[pipe.cls_key]['name'][r]) != str(b[0].cls[pipe.cls_key]['name'][r]) for r in rows))
                return {args.angle_mode: {'value': round(value, 3), 'unit': 'frames/s'}, other: {'value': round(K / dt, 3), 'unit': 'frames/s'},
                        'clusters_compared': n, 'class_names_that_differ': flips,
                        'note': "view direction angle of a cluster (pointcloud_utils.py:397): 'device' = correctly rounded atan2 on the GPU, 'reference' = "
                                "this host's float32 np.arctan2 of the device medians (one [C,3] read-back per frame); they differ by <= 1 ulp"}
            block('angle_modes', angle_modes)

            def resid16():
                # upstream's own GPU arithmetic (model.py:375-396 converts the whole tower to fp16: the residual stream too) as a
                # documented mode beside the default (fp32 residual stream, fp16 GEMM operands): a second tower handle created with
                # VG_VIT_RESID16=1, the same frames
                from vilgod_amd.clip_wrapper import ClipWrapper
                os.environ['VG_VIT_RESID16'] = '1'
                try:
                    clip16 = ClipWrapper(pipe._clip_cfg, '/nonexistent', device=dev, dtype=args.dtype)
                finally:
                    os.environ.pop('VG_VIT_RESID16', None)
                p2 = PseudoLabelPipeline(device=dev, vit_dtype=args.dtype, n_views=args.views, max_points=args.points + 1024, clip_model_path='/nonexistent',
                                         clip=clip16, box_mode=args.box_mode, vit_graph=args.vit_graph, angle_mode=args.angle_mode)
                fr = [f.to(dev) for f in host_frames] if args.input == 'resident' else host_frames
                settle(p2, args.points, args.objects)
                p2.new_sequence()
                p2.process_frames(fr[:W], [poses[i] for i in range(W)], poses[0], n_workers=inflight)
                p2.new_sequence()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = p2.process_frames(fr[W:W + K], [poses[W + i] for i in range(K)], poses[0], n_workers=inflight)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                p2._workers = None
                del p2, fr, clip16
                import gc
                gc.collect()
                torch.cuda.synchronize()
                n = flips = 0
                worst = 0.0
                for a, b in zip(outs0, res):
                    if a[2].shape == b[2].shape and a[2].numel():
                        worst = max(worst, float((a[2] - b[2]).abs().max()))
                    if np.array_equal(a[0].valid, b[0].valid) and pipe.cls_key in a[0].cls and pipe.cls_key in b[0].cls:
                        rows = np.flatnonzero(a[0].valid)
                        n += len(rows)
                        flips += int(sum(str(a[0].cls[pipe.cls_key]['name'][r]) != str(b[0].cls[pipe.cls_key]['name'][r]) for r in rows))
                return {'fp32_residual_stream': {'value': round(value, 3), 'unit': 'frames/s'},
                        'fp16_residual_stream': {'value': round(K / dt, 3), 'unit': 'frames/s'},
                        'max_abs_probability_difference': round(worst, 5), 'clusters_compared': n, 'class_names_that_differ': flips,
                        'note': 'VG_VIT_RESID16=1 at vg_vit_create: the residual stream in fp16 like the reference\'s CUDA run (EPI_BIAS_RESID_H epilogue: '
                                'half the read-modify-write bytes of out_proj / c_proj, no separate fp16 copy); NOT the default: against the fp32 oracle its '
                                'probability error is ~2.7e-3 (fp32 stream: ~6e-4), north_star asks for 1e-3.  Since the default tower runs its last block on the '
                                'class-token rows only (not implemented for this mode) the fp32 stream is also the faster one'}
            block('resid16', resid16)

            def f32_parity_mode():
                # the mode that meets north_star's 1e-3 bound on the logits by construction (fp32 tower: tests/test_vit.py <= 5e-5 against
                # the reference's model.py output; the integration goldens run in it): same frames, fewer steps (it is ~10x slower)
                from vilgod_amd.clip_wrapper import ClipWrapper
                n32 = min(K, 8)
                clip32 = ClipWrapper(pipe._clip_cfg, '/nonexistent', device=dev, dtype='f32')
                p2 = PseudoLabelPipeline(device=dev, vit_dtype='f32', n_views=args.views, max_points=args.points + 1024, clip_model_path='/nonexistent',
                                         clip=clip32, box_mode=args.box_mode, angle_mode=args.angle_mode)
                fr = [f.to(dev) for f in host_frames] if args.input == 'resident' else host_frames
                p2.new_sequence()
                p2.process_frames(fr[:min(W, 3)], [poses[i] for i in range(min(W, 3))], poses[0], n_workers=inflight)
                p2.new_sequence()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = p2.process_frames(fr[W:W + n32], [poses[W + i] for i in range(n32)], poses[0], n_workers=inflight)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                p2._workers = None
                del p2, fr, clip32
                import gc
                gc.collect()
                torch.cuda.synchronize()
                worst, n, flips = 0.0, 0, 0
                for a, b in zip(outs0, res):
                    if a[2].shape == b[2].shape and a[2].numel():
                        worst = max(worst, float((a[2] - b[2]).abs().max()))
                    if np.array_equal(a[0].valid, b[0].valid) and pipe.cls_key in a[0].cls and pipe.cls_key in b[0].cls:
                        rows = np.flatnonzero(a[0].valid)
                        n += len(rows)
                        flips += int(sum(str(a[0].cls[pipe.cls_key]['name'][r]) != str(b[0].cls[pipe.cls_key]['name'][r]) for r in rows))
                return {'value': round(n32 / dt, 3), 'unit': 'frames/s', 'steps': n32, 'dtype': 'f32',
                        'max_abs_probability_difference_to_the_metric_run': round(worst, 5), 'clusters_compared': n, 'class_names_that_differ': flips,
                        'note': 'vit_dtype=f32: the whole tower in fp32 (k_gemm_f32_mfma = v_mfma_f32_32x32x2_f32 on the matrix cores, k_attention_f32, k_layernorm), everything before it is the same '
                                'code as the metric\'s run; the first frames of the metric\'s stream'}
            block('f32_parity_mode', f32_parity_mode)

            def roofline_stages():
                # north_star asks for rocprof HBM GB/s evidence for clustering and renderer next to the MFMA figure: the stage kernels of the
                # committed rocprofv3 runs of this command (kernel trace for the time, separate PMC passes for the bytes; tools/collect_profiles.sh,
                # tools/summarize_profiles.py) -- read from profiles/, not measured in this run (PMC passes cannot run inside the timed region)
                spath = os.path.join(ROOT, 'profiles', 'stage_roofline.json')
                with open(spath) as f:
                    return json.load(f)
            block('roofline_stages', roofline_stages)
            block('views6', shape_block(args.points, args.objects, 6, 'BASELINE config 3 as written: 150k points, 6 rendered views'))
            block('dense200k', shape_block(200_000, 120, args.views, 'BASELINE config 5 shape: dense 200k-point frames, ~120 objects, fp16 ViT'))
        if args.full and world == 1 and not args.no_sequence_pass and not args.stage_times:
            def default_config_mode():
                # the reference's DEFAULT stage order (preprocessing.yaml:50-68 -- entropy scores over a 15-frame window + two-frame
                # 5-D clustering) on one coherent synthetic sequence, as a library call
                n_seq = max(48, K)
                sframes, sposes = synthetic.make_sequence(seed=0, n_frames=n_seq, n_points=args.points, n_objects=args.objects)
                sframes = [pipe.upload(f) for f in sframes]
                pipe.process_sequence(sframes[:4], sposes[:4], sposes[0], n_workers=inflight)
                torch.cuda.synchronize()
                ts = time.perf_counter()
                sres = pipe.process_sequence(sframes, sposes, sposes[0], n_workers=inflight)
                torch.cuda.synchronize()
                ts = time.perf_counter() - ts
                return {'value': round(n_seq / ts, 3), 'unit': 'frames/s', 'frames': n_seq,
                        'workload': ('mask_ground_points -> calculate_entropy_scores (15-frame window, skip 1) -> spatial_clustering n_frames=2 '
                                     '(5-D HDBSCAN + nearest-label transfer) -> filter -> classification -> boxes on one coherent '
                                     f'synthetic sequence of {n_seq} frames x {args.points} points'),
                        'labelled_per_frame': round(sum(len(r[1]['name']) for r in sres) / n_seq, 1),
                        'moving_clusters_per_frame': round(sum(int((~r[0].static).sum()) for r in sres) / n_seq, 1)}
            block('default_config_mode', default_config_mode)
        if extras and args.cli_frames > 0:
            def cli_mode():
                # the entry point itself (north_star's boundary): tools/preprocess_data.py preprocessor=waymo, default stage list, on
                # several sequences of the benchmark workload (a real run walks 798 of them: what counts is the steady state, in which a
                # sequence's state pickle is written by the helper process and its host-only tail runs under the next sequence's GPU
                # stages).  seed_stride=0: every sequence is the SAME world under its own name, generated once.
                # Run as a CHILD process, like a user would: this process has built a dozen pipeline objects by now (streams, handles,
                # allocator pools) and the entry point read 8 % lower inside it than on its own; the GPU is idle here meanwhile.
                nseq = max(1, int(args.cli_sequences))
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'time_cli.py'), str(args.cli_frames), str(args.points),
                                    f'dataset.SYNTHETIC.objects_per_frame={args.objects}', f'device.frames_in_flight={inflight}',
                                    f'device.box_mode={args.box_mode}'],
                                   env=dict(os.environ, SEQUENCES=str(nseq), SEED_STRIDE='0', TIME_CLI_JSON='1'), capture_output=True, text=True, timeout=900)
                total = time.perf_counter() - t0
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith('TIME_CLI_JSON ')]
                if r.returncode != 0 or not lines:
                    raise RuntimeError(f'tools/time_cli.py failed (rc {r.returncode}): {r.stderr[-600:]}')
                run = json.loads(lines[-1][len('TIME_CLI_JSON '):])
                seqs = run['sequences']
                frames = sum(q['frames'] for q in seqs)
                later = seqs[1:] or seqs
                # the same entry point as TWO processes on this GPU (device.processes_per_gpu=2: whole sequences per process, nothing exchanged
                # until the final evaluation; one's host-only stages run under the other's frame pass), on twice the sequences
                two = None
                if nseq >= 2:
                    r2 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'time_cli.py'), str(args.cli_frames), str(args.points),
                                         f'dataset.SYNTHETIC.objects_per_frame={args.objects}', f'device.box_mode={args.box_mode}', 'device.frames_in_flight=4'],
                                        env=dict(os.environ, SEQUENCES=str(2 * nseq), SEED_STRIDE='0', TIME_CLI_JSON='1', PROCS='2'),
                                        capture_output=True, text=True, timeout=900)
                    l2 = [ln for ln in r2.stdout.splitlines() if ln.startswith('TIME_CLI_JSON ')]
                    if r2.returncode != 0 or not l2:             # (must not cost the one-process figure)
                        two = {'error': f'tools/time_cli.py PROCS=2 failed (rc {r2.returncode}): {(r2.stderr or r2.stdout)[-600:]}'}
                    else:
                        q2 = json.loads(l2[-1][len('TIME_CLI_JSON '):])
                        f2 = sum(q['frames'] for q in q2['sequences'])
                        two = {'value': round(f2 / q2['loop_seconds'], 3), 'unit': 'frames/s', 'frames': f2, 'sequences': len(q2['sequences']), 'processes': 2,
                                'frames_in_flight_per_process': 4, 'ms_per_frame': round(1000.0 * q2['loop_seconds'] / f2, 2),
                                'window_seconds': round(q2['window_seconds'], 2), 'generator_seconds_excluded': round(q2['generator_seconds'], 2),
                                'loop_seconds_per_rank': [round(x, 2) for x in q2['loop_seconds_per_rank']],
                                'note': ('tools/preprocess_data.py device.processes_per_gpu=2 (started through torch.distributed.run, gloo group): rank r walks '
                                         'sequences r, r + 2, ...; value = all frames / (first rank\'s loop start to last rank\'s loop end, minus the synthetic '
                                         'generator every rank runs at the start of its loop); both pickle families equal the one-process run\'s '
                                         '(tests/test_cli.py::test_cli_sequence_sharding_equals_one_rank)')}
                return {'two_processes_per_gpu': two, 'value': round(frames / run['loop_seconds'], 3), 'unit': 'frames/s', 'frames': frames, 'sequences': len(seqs),
                        'ms_per_frame': round(1000.0 * run['loop_seconds'] / frames, 2),
                        'state_write_wait_seconds': round(run.get('state_write_wait_seconds', 0.0), 3),
                        'per_sequence': [{'front_ms_per_frame': round(1000.0 * q['front_seconds'] / q['frames'], 2),
                                          'tail_ms_per_frame': round(1000.0 * q['back_seconds'] / q['frames'], 2)} for q in seqs],
                        'stage_ms_per_frame': {k: round(sum(q['stage_ms_per_frame'].get(k, 0.0) for q in later) / len(later), 2)
                                               for k in later[0]['stage_ms_per_frame']},
                        'whole_command_seconds': round(total, 1),
                        'workload': (f'tools/preprocess_data.py preprocessor=waymo on {len(seqs)} coherent synthetic sequences of {seqs[0]["frames"]} frames x '
                                     f'{args.points} points (the same world under {len(seqs)} names), the reference\'s default 9-stage pipeline_active (ground, '
                                     'entropy scores, two-frame clustering, filters, tracking, classification, boxes, label propagation, '
                                     'evaluate_sequence); value = all frames / wall time of the sequence loop, from "first sequence selected" to "every '
                                     'pickle of the last sequence on disk" (the background state write included; the synthetic generator, which stands '
                                     'for disk IO, excluded); stage_ms_per_frame = mean over the sequences after the first; tail = the host-only stages '
                                     'that run on a thread under the next sequence\'s GPU stages; whole_command_seconds adds start-up, the generator and '
                                     'the AP evaluation over the generator\'s ground truth')}
            block('cli_mode', cli_mode)
        if args.full and world == 1 and not args.no_cpu_baseline:
            block('cpu_baseline', cpu_baseline)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
