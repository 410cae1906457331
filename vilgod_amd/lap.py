"""Linear assignment on the GPU: scipy's `linear_sum_assignment` call shape over vg_lap_groups (csrc/lap.hip).

    from vilgod_amd.lap import linear_sum_assignment      # instead of scipy.optimize.linear_sum_assignment
    row_ind, col_ind = linear_sum_assignment(cost)         # CUDA tensor [n, m] -> int64 CUDA tensors; numpy in -> numpy out

The reference reaches that routine in src/datasets/waymo_eval.py:111 (the metric's matcher) and src/utils/tracking_utils.py:23-51.
The solver is shortest augmenting paths with duals in float64, as scipy's; where several assignments share the smallest total it
returns one of them by its own tie rule (include/vilgod_hip.h), not necessarily scipy's.
`lap_groups` solves many independent problems in one launch, each with optional "stay unassigned" price, row order and snapshots
after listed prefixes of the rows (the evaluation: one group per frame and object type, one snapshot per distinct kept set);
`lap_groups_host` is the same per-column code on the CPU (vg_lap_groups_host), bit for bit.  A numpy matrix handed to
`linear_sum_assignment` is solved by the host form, a CUDA tensor by the kernel: the input picks the form, neither stands in for the
other.
"""
import ctypes

import numpy as np

from ._lib import lib, check, ptr, stream_ptr, _DEFINES

LAP_MAX = _DEFINES['LAP_MAX']
SOLVED, INFEASIBLE, INVALID, BAD_TABLE = 0, 1, 2, -1


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _tables(cost_len, cost_off, row_off, col_off, order_len, prefixes):
    """The host side of both forms: the offset tables as the ABI wants them, the snapshots' places and the size bounds."""
    row_off, col_off = np.ascontiguousarray(row_off, np.int32), np.ascontiguousarray(col_off, np.int32)
    cost_off = np.ascontiguousarray(cost_off, np.int64)
    if row_off.ndim != 1 or row_off.shape != col_off.shape or len(row_off) < 1 or cost_off.shape != (len(row_off) - 1,):
        raise ValueError('row_off and col_off must be 1-D of equal length G + 1, cost_off of length G')
    n_groups = len(row_off) - 1
    n, m = np.diff(row_off.astype(np.int64)), np.diff(col_off.astype(np.int64))
    if prefixes is None:
        prefix = prefix_off = None
        per_snap = np.maximum(n, 0)
    else:
        if len(prefixes) != n_groups:
            raise ValueError('prefixes must hold one list per group')
        counts = [len(p) for p in prefixes]
        prefix_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        prefix = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in prefixes] + [np.zeros(0, np.int64)]),
                                      np.int32)
        per_snap = np.repeat(np.maximum(n, 0), counts)
    ends = np.cumsum(per_snap)
    match_off = np.ascontiguousarray(ends - per_snap, np.int64)
    t = {'cost_off': cost_off, 'row_off': row_off, 'col_off': col_off, 'prefix': prefix, 'prefix_off': prefix_off, 'match_off': match_off,
         'n_groups': n_groups, 'n_snaps': len(match_off), 'match_len': int(ends[-1]) if len(ends) else 0,
         'max_rows': int(max(n.max(), 0)) if n_groups else 0, 'max_cols': int(max(m.max(), 0)) if n_groups else 0,
         'snap_off': np.arange(n_groups + 1, dtype=np.int64) if prefix_off is None else prefix_off.astype(np.int64),
         'cost_len': int(cost_len), 'n_rows': int(order_len)}
    return t


def lap_groups_host(cost, cost_off, row_off, col_off, unassigned_cost=np.inf, order=None, prefixes=None):
    """numpy form of `lap_groups` through the host entry point: the same arguments as arrays, the same four results as arrays."""
    cost = np.ascontiguousarray(np.asarray(cost, np.float64).reshape(-1))
    order = None if order is None else np.ascontiguousarray(np.asarray(order).reshape(-1), np.int32)
    t = _tables(len(cost), cost_off, row_off, col_off, 0 if order is None else len(order), prefixes)
    match = np.full(t['match_len'], -2, np.int32)
    status = np.full(t['n_groups'], -2, np.int32)
    check(lib.vg_lap_groups_host(_np_ptr(cost), t['cost_len'], _np_ptr(t['cost_off']), _np_ptr(t['row_off']), _np_ptr(t['col_off']),
                                 t['n_groups'], t['n_rows'], t['max_rows'], t['max_cols'], float(unassigned_cost), _np_ptr(order),
                                 _np_ptr(t['prefix']), _np_ptr(t['prefix_off']), t['n_snaps'], _np_ptr(t['match_off']), t['match_len'],
                                 _np_ptr(match), _np_ptr(status)), 'vg_lap_groups_host')
    return match, t['match_off'], t['snap_off'], status


def lap_groups(cost, cost_off, row_off, col_off, unassigned_cost=np.inf, order=None, prefixes=None, stream=None):
    """Many independent assignment problems in ONE launch, everything left on the device.
    cost: flat float64 CUDA tensor; group g's row-major [n_g, m_g] matrix starts at cost_off[g], n_g = row_off[g+1] - row_off[g],
    m_g = col_off[g+1] - col_off[g] (the tables of iou.iou_groups: its result can be passed on as it is).
    unassigned_cost: the price at which a row may stay without a column (inf: it may not).
    order: flat int32 (CUDA tensor or array), entries row_off[g] .. row_off[g+1] a permutation of 0 .. n_g - 1: the order in which the
    rows enter.  prefixes: one strictly ascending list of prefix lengths (1 .. n_g) per group; None: one snapshot after the last row.
    -> (match, match_off, snap_off, status): match flat int32 CUDA tensor, snapshot s = match[match_off[s] : match_off[s] + n_g], the
    column of every row (-1: none, or not yet entered); group g's snapshots are s = snap_off[g] .. snap_off[g+1] - 1, in the order of
    its prefixes; status int32 CUDA tensor [G] (SOLVED, INFEASIBLE, INVALID, BAD_TABLE; a group that is not SOLVED has -1 throughout).
    `stream`: a torch stream on which the costs are ready (default: the current one)."""
    import torch
    if not (torch.is_tensor(cost) and cost.is_cuda):
        raise ValueError('lap_groups takes a CUDA tensor (lap_groups_host is the CPU form)')
    if cost.dtype != torch.float64:
        raise ValueError(f'costs must be float64 (got {cost.dtype})')
    dev = cost.device
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        cost = cost.reshape(-1).contiguous()
        if order is not None:
            order = (order if torch.is_tensor(order) else torch.from_numpy(np.ascontiguousarray(np.asarray(order).reshape(-1), np.int32)))
            order = order.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        t = _tables(cost.numel(), cost_off, row_off, col_off, 0 if order is None else order.numel(), prefixes)
        up = {k: None if t[k] is None else torch.from_numpy(t[k]).to(dev) for k in ('cost_off', 'row_off', 'col_off', 'prefix', 'prefix_off',
                                                                                   'match_off')}
        match = torch.full((t['match_len'],), -2, dtype=torch.int32, device=dev)
        status = torch.full((t['n_groups'],), -2, dtype=torch.int32, device=dev)
        check(lib.vg_lap_groups(ptr(cost), t['cost_len'], ptr(up['cost_off']), ptr(up['row_off']), ptr(up['col_off']), t['n_groups'],
                                t['n_rows'], t['max_rows'], t['max_cols'], float(unassigned_cost), ptr(order), ptr(up['prefix']),
                                ptr(up['prefix_off']), t['n_snaps'], ptr(up['match_off']), t['match_len'], ptr(match), ptr(status),
                                stream_ptr(stream)), 'vg_lap_groups')
    return match, t['match_off'], t['snap_off'], status


def linear_sum_assignment(cost, maximize=False):
    """scipy.optimize.linear_sum_assignment: [n, m] costs -> (row_ind, col_ind), min(n, m) pairs with the rows ascending, int64.
    A CUDA tensor is solved by the kernel and gives CUDA tensors; anything else goes through numpy and the host form."""
    import torch
    on_device = torch.is_tensor(cost) and cost.is_cuda
    c = cost.detach() if torch.is_tensor(cost) else np.asarray(cost)
    if c.ndim != 2:
        raise ValueError(f'expected a matrix (2-D array), got a {c.ndim} array')
    if not on_device:
        c = np.asarray(c.numpy() if torch.is_tensor(c) else c)
        if not (np.issubdtype(c.dtype, np.number) or c.dtype == np.bool_):
            raise ValueError(f'expected a matrix containing numerical entries, got {c.dtype}')
        c = c.astype(np.float64)
    else:
        c = c.to(torch.float64)
    if maximize:
        c = -c
    transposed = c.shape[0] > c.shape[1]
    if transposed:
        c = c.T
    n, m = c.shape
    if on_device:
        match, _, _, status = lap_groups(c.contiguous().reshape(-1), [0], [0, n], [0, m])
        st = int(status.cpu()[0])
    else:
        match, _, _, status = lap_groups_host(np.ascontiguousarray(c).reshape(-1), [0], [0, n], [0, m])
        st = int(status[0])
    if st == INVALID:
        raise ValueError('matrix contains invalid numeric entries')
    if st == INFEASIBLE:
        raise ValueError('cost matrix is infeasible')
    if st != SOLVED:
        raise RuntimeError(f'vg_lap_groups: status {st}')
    if on_device:
        rows, cols = torch.arange(n, dtype=torch.int64, device=match.device), match.to(torch.int64)
        if transposed:
            cols, by = torch.sort(cols)
            rows, cols = cols, rows[by]
    else:
        rows, cols = np.arange(n, dtype=np.int64), match.astype(np.int64)
        if transposed:
            by = np.argsort(cols, kind='stable')
            rows, cols = cols[by], rows[by]
    return rows, cols
