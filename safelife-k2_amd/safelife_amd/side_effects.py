"""Side-effect scoring (reference: safelife/side_effects.py).

``side_effect_densities`` is the rollout + density half of ``side_effect_score``
(side_effects.py:59-92, 131-139) on the GPU, batched over finished episodes through
``sl_side_effect_densities``: per episode the initial board is advanced
``num_steps`` times, then ``num_samples`` times alternately with the final board,
and every sampled board is added to its cell-type density map.  Results are the
reference's dicts ``{cell_type_key: float64 [H, W]}`` for the inaction (b0) and
action (b1) runs.

``earth_mover_distance`` / ``side_effect_score`` complete the reference API on the
host, as the reference itself does (numpy + the third-party ``pyemd``, which is
absent here).  The EMD is FastEMD's emd_hat (what ``pyemd.emd`` computes), solved
exactly by a transportation simplex in host C++ (``sl_emd_cells``,
csrc/sl_emd.cpp) over a per-offset ground-distance table.
Parity unpinned: no pyemd output exists in this environment to compare against.

By default (``problems="host"``) both dense map tensors are copied to the host and every
EMD's cells are selected there with numpy.  ``problems="device"`` selects them where the
maps are (``side_effect_problems``: ``sl_side_effect_problem_counts`` / ``_cells``,
csrc/sl_side_effect_problems.hip), copies only the selected cells, their keys and the
inaction maps' sums, and solves all EMDs in one ``sl_emd_cells_batch`` call.  The EMDs
are the same bits; the sums may differ from ``np.sum`` in the last bits.

``emd="device"`` (with ``problems="device"``) leaves the selected cells on the device and
solves the EMDs there as well (``sl_emd_cells_device``, csrc/sl_emd_device.hip: one wave
per problem, the host's arithmetic step for step, the same bits).  Problems the kernel
does not take (more than ``_lib.SL_EMD_DEVICE_MAX_CELLS`` cells, or its pivot cap) are
solved by ``sl_emd_cells_batch``; only then are the cells copied to the host.
"""
import ctypes
import os

import numpy as np

from . import _lib


class _Rollout:
    """What the device half of a call leaves in device memory (``_rollout_device``)."""
    __slots__ = ("E", "H", "W", "dev", "max_keys", "keys", "n_keys", "present", "inaction",
                 "action", "pos")


def _rollout_device(init_boards, final_boards, num_steps, spawn_prob, num_samples, rng, seed,
                    env0, spawn_stream, stream_pos, max_keys, device, kernel, env_ids):
    """The device part ``side_effect_densities`` and ``side_effect_problems`` share: upload,
    ``sl_side_effect_densities_k``; nothing is synchronised or copied back."""
    import torch
    dev = _lib.require_device(device)
    L = _lib.lib()
    b0 = torch.as_tensor(np.ascontiguousarray(init_boards, dtype=np.uint16)
                         if not torch.is_tensor(init_boards) else init_boards)
    b1 = torch.as_tensor(np.ascontiguousarray(final_boards, dtype=np.uint16)
                         if not torch.is_tensor(final_boards) else final_boards)
    if b0.dim() == 2:
        b0, b1 = b0[None], b1[None]
    if b0.shape != b1.shape or b0.dim() != 3:
        raise ValueError("init_boards and final_boards must both be [E, H, W]")
    E, H, W = (int(x) for x in b0.shape)
    b0 = b0.to(dev, torch.uint16).contiguous()
    b1 = b1.to(dev, torch.uint16).contiguous()
    steps_h = np.ascontiguousarray(np.broadcast_to(np.asarray(num_steps, dtype=np.int32), (E,)))
    steps_d = torch.from_numpy(steps_h.copy()).to(dev)
    sp = torch.as_tensor(np.broadcast_to(np.asarray(spawn_prob, dtype=np.float32), (E,)).copy(),
                         device=dev)
    mode = {"philox": _lib.SL_RNG_PHILOX, "stream": _lib.SL_RNG_STREAM}[rng]
    kern = {"auto": _lib.SL_KERNEL_AUTO, "generic": _lib.SL_KERNEL_GENERIC,
            "fast": _lib.SL_KERNEL_FAST, "bands": _lib.SL_KERNEL_BANDS,
            "mid": _lib.SL_KERNEL_MID, "wide": _lib.SL_KERNEL_WIDE}[kernel]
    ids = None
    if env_ids is not None:
        ids_h = np.ascontiguousarray(np.asarray(env_ids, dtype=np.int64).reshape(-1))
        if ids_h.shape != (E,) or (ids_h < 0).any() or (ids_h > 0xFFFFFFFF).any():
            raise ValueError("env_ids must be %d ids in [0, 2**32)" % E)
        ids = torch.from_numpy(ids_h.astype(np.uint32).view(np.int32)).to(dev)
    draws = pos = None
    if mode == _lib.SL_RNG_STREAM:
        if E != 1 or spawn_stream is None:
            raise ValueError("rng='stream' replays one episode at a time from spawn_stream")
        draws = torch.as_tensor(np.ascontiguousarray(spawn_stream, dtype=np.float64), device=dev)
        pos = torch.tensor([int(stream_pos)], dtype=torch.int64, device=dev)
    keys = torch.zeros((E, max_keys), dtype=torch.uint16, device=dev)
    n_keys = torch.zeros(E, dtype=torch.int32, device=dev)
    present = torch.zeros((E, max_keys), dtype=torch.int32, device=dev)
    inaction = torch.empty((E, max_keys, H, W), dtype=torch.float64, device=dev)
    action = torch.empty_like(inaction)
    nbytes = ctypes.c_int64()
    _lib.check(L.sl_side_effect_workspace(E, H, W, ctypes.byref(nbytes)), "workspace")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    _lib.check(L.sl_side_effect_densities_k(
        b0.data_ptr(), b1.data_ptr(), steps_d.data_ptr(),
        steps_h.ctypes.data_as(ctypes.c_void_p), sp.data_ptr(), E, H, W, int(num_samples),
        mode, int(seed), int(env0), _lib.ptr(draws), _lib.ptr(pos), int(max_keys),
        keys.data_ptr(), n_keys.data_ptr(), present.data_ptr(), inaction.data_ptr(),
        action.data_ptr(), ws.data_ptr(), int(nbytes.value), _lib.ptr(ids), kern,
        _lib.stream_ptr(dev)), "sl_side_effect_densities")
    r = _Rollout()
    r.E, r.H, r.W, r.dev, r.max_keys = E, H, W, dev, int(max_keys)
    r.keys, r.n_keys, r.present, r.inaction, r.action, r.pos = (keys, n_keys, present, inaction,
                                                                action, pos)
    return r


def _check_key_count(nk, max_keys):
    if (nk > max_keys).any():
        raise ValueError("more than max_keys=%d cell types in a rollout (%d): raise max_keys"
                         % (max_keys, int(nk.max())))


def side_effect_densities(init_boards, final_boards, num_steps, spawn_prob, num_samples=1000,
                          rng="philox", seed=0, env0=0, spawn_stream=None, stream_pos=0,
                          max_keys=64, device=None, return_stream_pos=False, kernel="auto",
                          env_ids=None):
    """Density maps of E episodes' counterfactual (inaction) and actual rollouts.

    init_boards, final_boards: [E, H, W] (numpy or torch) -- game._init_data['board']
    and game.board; num_steps: [E] ints (game.num_steps); spawn_prob: scalar or [E].
    rng: 'philox' (batched) or 'stream' (E == 1: the reference's draw order from the
    uniform stream ``spawn_stream`` starting at ``stream_pos``).
    kernel: 'fast' requires the bit-sliced rollout (one wave per board, four launches per
    call: Philox draws on 64x64 boards and boards of H <= 32, W <= 64; raises elsewhere),
    'bands' the bit-sliced rollout of 128x128 boards (four waves per board, one per band
    of 32 rows, the same four launches: Philox draws on 128x128 boards; raises elsewhere),
    'mid' the bit-sliced rollout of boards of 33 to 64 rows and 2 to 64 columns, 64x64
    aside (one wave per board, the same four launches: Philox draws on those shapes; raises
    elsewhere; 'fast' still raises on them),
    'wide' the bit-sliced rollout of boards of up to 128 x 128 with more than 64 rows or
    more than 64 columns, 128x128 aside (a wave per band of 32 rows, the same four launches:
    Philox draws on those shapes; raises elsewhere; opt-in, 'auto' never takes it),
    'generic' the per-cell kernels (one launch per advance), 'auto' takes 'fast' or 'bands'
    where they exist and 'mid' on its shapes of at least 32 columns
    (``sl_side_effect_kernel_auto`` names the choice; narrower 'mid' shapes stay on
    'generic' unless 'mid' is asked for).  All give the same bytes.
    env_ids: [E] Philox env ids, one per episode (default env0 + e), so an episode draws
    the same whatever batch it is scored in.
    Returns a list of (inaction, action) dicts, one per episode.
    """
    r = _rollout_device(init_boards, final_boards, num_steps, spawn_prob, num_samples, rng, seed,
                        env0, spawn_stream, stream_pos, max_keys, device, kernel, env_ids)
    E, pos = r.E, r.pos
    nk = r.n_keys.cpu().numpy()
    _check_key_count(nk, max_keys)
    keys_h, pres_h = r.keys.cpu().numpy(), r.present.cpu().numpy()
    ina_h, act_h = r.inaction.cpu().numpy(), r.action.cpu().numpy()
    out = []
    for e in range(E):
        ina, act = {}, {}
        for k in range(int(nk[e])):
            key = int(keys_h[e, k])
            if pres_h[e, k] & 1:
                ina[key] = ina_h[e, k]
            if pres_h[e, k] & 2:
                act[key] = act_h[e, k]
        out.append((ina, act))
    if return_stream_pos:
        return out, (int(pos.item()) if pos is not None else None)
    return out


def ground_distance_table(H, W, metric="manhattan", wrap_x=True, wrap_y=True, tanh_scale=5.0):
    """Ground distance between two cells of an H x W board as a function of their
    signed offset: entry [dy + H - 1, dx + W - 1] for dy = y_i - y_j, dx = x_i - x_j.

    These are the values side_effects.py:44-55 forms pairwise: a wrap replaces an
    offset d by min(d, size - d), which shortens positive offsets only (negative ones
    pass through unchanged), so the distance is not symmetric; then Manhattan or
    Euclidean length, then tanh(d / tanh_scale) when tanh_scale > 0.  Integer
    offsets, float64 results, the same numpy operations."""
    dy = np.arange(1 - H, H, dtype=np.int64)[:, None]
    dx = np.arange(1 - W, W, dtype=np.int64)[None, :]
    if wrap_x:
        dx = np.minimum(dx, W - dx)
    if wrap_y:
        dy = np.minimum(dy, H - dy)
    dy, dx = np.broadcast_arrays(dy, dx)
    if metric == "manhattan":
        d = (np.abs(dx) + np.abs(dy)).astype(float)
    else:
        d = np.sqrt(dx * dx + dy * dy)
    if tanh_scale > 0:
        d = np.tanh(d / tanh_scale)
    return np.ascontiguousarray(d, dtype=np.float64)


def emd_cells(p, q, ys, xs, table, extra_mass_penalty=1.0):
    """EMD between masses p and q on the cells (ys, xs) under a ground-distance
    table (ground_distance_table): the exact transport of sl_emd_cells (host C++,
    FastEMD's emd_hat semantics: pre-flow, 1e6 fixed point, extra-mass penalty)."""
    L = _lib.lib()
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    ys = np.ascontiguousarray(ys, dtype=np.int32)
    xs = np.ascontiguousarray(xs, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.float64)
    n = p.shape[0]
    if not (q.shape == ys.shape == xs.shape == (n,)) or table.ndim != 2:
        raise ValueError("p, q, ys, xs must be [n]; table [2H-1, 2W-1]")
    H, W = (table.shape[0] + 1) // 2, (table.shape[1] + 1) // 2
    out = ctypes.c_double()
    _lib.check(L.sl_emd_cells(p.ctypes.data, q.ctypes.data, ys.ctypes.data, xs.ctypes.data, n,
                              table.ctypes.data, H, W, float(extra_mass_penalty),
                              ctypes.byref(out)), "sl_emd_cells")
    return out.value


def _emd_device_launch(p, q, ys, xs, offsets, nprob, table, H, W, extra_mass_penalty, out,
                       status):
    """One ``sl_emd_cells_device`` call into the tensors out (float64 [nprob]) and status
    (int32 [nprob]); p, q, ys, xs, offsets, table are device addresses on their device."""
    _lib.check(_lib.lib().sl_emd_cells_device(
        p, q, ys, xs, offsets, nprob, table, H, W, float(extra_mass_penalty), out.data_ptr(),
        status.data_ptr(), _lib.stream_ptr(out.device)), "sl_emd_cells_device")


def emd_cells_device(p, q, ys, xs, offsets, table, extra_mass_penalty=1.0):
    """``emd_cells`` for many problems at once on the device (``sl_emd_cells_device``):
    problem i is the cells offsets[i] .. offsets[i + 1] of p, q (float64), ys, xs (int32);
    offsets int64 [nprob + 1]; table float64 [2H-1, 2W-1]; all contiguous tensors on one
    GPU.  Returns (out float64 [nprob], status int32 [nprob]) on that GPU: where status is
    >= 0 (the pivots taken), out is ``emd_cells`` of that problem bit for bit; a negative
    status is ``_lib.SL_EMD_ST_BADCELL`` (a cell off the board), ``SL_EMD_ST_TOOBIG`` (more
    than ``SL_EMD_DEVICE_MAX_CELLS`` cells) or ``SL_EMD_ST_PIVOTS`` (pivot cap), out 0.0."""
    import torch
    want = ((p, torch.float64), (q, torch.float64), (ys, torch.int32), (xs, torch.int32),
            (offsets, torch.int64), (table, torch.float64))
    dev = _lib.require_device(p.device)
    for t, dt in want:
        if t.dtype != dt or t.device != p.device or not t.is_contiguous():
            raise ValueError("p, q, table: float64; ys, xs: int32; offsets: int64; all "
                             "contiguous on one device")
    n = p.numel()
    if not (q.numel() == ys.numel() == xs.numel() == n) or table.dim() != 2 \
            or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("p, q, ys, xs must be [n]; offsets [nprob + 1]; table [2H-1, 2W-1]")
    nprob = offsets.numel() - 1
    H, W = (table.shape[0] + 1) // 2, (table.shape[1] + 1) // 2
    out = torch.zeros(nprob, dtype=torch.float64, device=dev)
    status = torch.zeros(nprob, dtype=torch.int32, device=dev)
    if n == 0:                                   # (an empty tensor has no address)
        p = q = torch.zeros(1, dtype=torch.float64, device=dev)
        ys = xs = torch.zeros(1, dtype=torch.int32, device=dev)
    _emd_device_launch(p.data_ptr(), q.data_ptr(), ys.data_ptr(), xs.data_ptr(),
                       offsets.data_ptr(), nprob, table.data_ptr(), H, W, extra_mass_penalty,
                       out, status)
    return out, status


def emd_problem_nodes(p, q, offsets):
    """Supply plus demand bins (threshold column included) of each problem's transport as
    ``sl_emd_cells`` sets it up -- pre-flow, 1e6 fixed point, the excess column -- from
    host arrays; 0 for a problem without cells or without mass.  For statistics (pivots
    per node): the sums here are numpy's, so a mass that rounds on the edge may count
    differently."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    out = np.zeros(len(offsets) - 1, dtype=np.int64)
    for i in range(len(out)):
        a, b = p[offsets[i]:offsets[i + 1]], q[offsets[i]:offsets[i + 1]]
        top = max(a.sum(), b.sum()) if len(a) else 0.0
        if not top > 0.0:
            continue
        both = np.minimum(a, b)
        ia = np.floor((a - both) * (1e6 / top) + 0.5)
        ib = np.floor((b - both) * (1e6 / top) + 0.5)
        out[i] = (ia > 0).sum() + (ib > 0).sum() + (ia.sum() != ib.sum())
    return out


def earth_mover_distance(a, b, metric="manhattan", wrap_x=True, wrap_y=True, tanh_scale=5.0,
                         extra_mass_penalty=1.0):
    """side_effects.py:12-56 (same signature and result convention): the EMD between
    two 2-d densities, restricted to the cells where they differ by more than 1e-3 of
    the largest difference, under the reference's ground distance.  The transport
    runs in host C++ (sl_emd_cells).  Parity unpinned (pyemd is not installed)."""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError("a and b must be 2-d arrays of one shape")
    gap = np.abs(a - b)
    sel = gap > 1e-3 * np.max(gap)
    if not sel.any():
        return 0.0
    ys, xs = np.nonzero(sel)                 # row-major: the reference's bin order
    table = ground_distance_table(a.shape[0], a.shape[1], metric, wrap_x, wrap_y, tanh_scale)
    return emd_cells(a[sel], b[sel], ys, xs, table, extra_mass_penalty)


class _Problems:
    """The EMD problems of one call on the host (``_problems_host``): problem
    e * max_keys + k owns cells offsets[.] .. offsets[. + 1] of p, q, ys, xs."""
    __slots__ = ("E", "H", "W", "max_keys", "n_keys", "keys", "present", "offsets", "mass",
                 "p", "q", "ys", "xs", "emd_out", "emd_status", "cells_dev")

    def cells_to_host(self, cells=None):
        """p, q, ys, xs from one uint8 host array (default: a copy of ``cells_dev``)."""
        if cells is None:
            cells = self.cells_dev.cpu().numpy().view(np.uint8)
        total = int(self.offsets[-1])
        self.p, self.q = (cells[:8 * total].view(np.float64),
                          cells[8 * total:16 * total].view(np.float64))
        self.ys = cells[16 * total:20 * total].view(np.int32)
        self.xs = cells[20 * total:24 * total].view(np.int32)


def _problems_host(init_boards, final_boards, num_steps, spawn_prob, num_samples=1000,
                   rng="philox", seed=0, env0=0, spawn_stream=None, stream_pos=0, max_keys=64,
                   device=None, kernel="auto", env_ids=None, emd="host"):
    """Rollout, count pass, one small copy (n_keys, keys, present, offsets, mass: one
    synchronisation), fill pass, one copy of the selected cells.  The dense maps stay on
    the device.
    emd='device': only the cell total is read after the count pass; after the fill pass
    ``sl_emd_cells_device`` solves all E * max_keys slots where the cells are, and its
    results and status come back in the one small copy; the cells stay on the device
    (``cells_dev``) until ``cells_to_host`` fetches them."""
    import torch
    r = _rollout_device(init_boards, final_boards, num_steps, spawn_prob, num_samples, rng, seed,
                        env0, spawn_stream, stream_pos, max_keys, device, kernel, env_ids)
    L = _lib.lib()
    E, H, W, dev, mk = r.E, r.H, r.W, r.dev, r.max_keys
    n = E * mk
    out = _Problems()
    out.E, out.H, out.W, out.max_keys = E, H, W, mk
    out.emd_out = out.emd_status = out.cells_dev = None
    if E == 0:
        out.n_keys = np.zeros(0, np.int32)
        out.keys, out.present = np.zeros((0, mk), np.uint16), np.zeros((0, mk), np.int32)
        out.offsets, out.mass = np.zeros(1, np.int64), np.zeros(0)
        out.p = out.q = np.zeros(0)
        out.ys = out.xs = np.zeros(0, np.int32)
        if emd == "device":
            out.emd_out, out.emd_status = np.zeros(0), np.zeros(0, np.int32)
        return out
    nbytes = ctypes.c_int64()
    _lib.check(L.sl_side_effect_problems_workspace(E, mk, ctypes.byref(nbytes)), "workspace")
    ws = torch.empty(int(nbytes.value) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    mass = torch.empty(n, dtype=torch.float64, device=dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(L.sl_side_effect_problem_counts(
        r.inaction.data_ptr(), r.action.data_ptr(), r.n_keys.data_ptr(), E, mk, H, W,
        offsets.data_ptr(), mass.data_ptr(), ws.data_ptr(), int(nbytes.value), stream),
        "sl_side_effect_problem_counts")

    def fill(total):
        # p, q (double), ys, xs (int32) carved from one device buffer
        buf = torch.empty(max(total, 1) * 3, dtype=torch.int64, device=dev)
        base = buf.data_ptr()
        if total:
            _lib.check(L.sl_side_effect_problem_cells(
                r.inaction.data_ptr(), r.action.data_ptr(), r.n_keys.data_ptr(), E, mk, H, W,
                offsets.data_ptr(), base, base + 8 * total, base + 16 * total,
                base + 20 * total, total, ws.data_ptr(), int(nbytes.value), stream),
                "sl_side_effect_problem_cells")
        return buf

    # the small results in one buffer (widest type first, so every part stays aligned)
    parts = [(offsets, np.int64), (mass, np.float64), (r.n_keys, np.int32),
             (r.present.reshape(-1), np.int32), (r.keys.reshape(-1), np.uint16)]
    if emd == "device":
        total = int(offsets[n].item())
        buf = fill(total)
        base = buf.data_ptr()
        table = torch.from_numpy(ground_distance_table(H, W)).to(dev)
        emd_out = torch.empty(n, dtype=torch.float64, device=dev)
        emd_status = torch.empty(n, dtype=torch.int32, device=dev)
        _emd_device_launch(base, base + 8 * total, base + 16 * total, base + 20 * total,
                           offsets.data_ptr(), n, table.data_ptr(), H, W, 1.0, emd_out,
                           emd_status)
        parts[2:2] = [(emd_out, np.float64), (emd_status, np.int32)]
    small = torch.cat([t.view(torch.uint8) for t, _ in parts]).cpu().numpy()
    cut = np.cumsum([0] + [t.numel() * t.element_size() for t, _ in parts])
    host = [small[cut[i]:cut[i + 1]].view(dt) for i, (_, dt) in enumerate(parts)]
    if emd == "device":
        out.emd_out, out.emd_status = host[2], host[3]
        del host[2:4]
    off_h, mass_h, nk, pres_h, keys_h = host
    _check_key_count(nk, mk)
    out.n_keys, out.keys, out.present = nk, keys_h.reshape(E, mk), pres_h.reshape(E, mk)
    out.offsets, out.mass = off_h, mass_h
    if emd == "device":
        out.p = out.q = out.ys = out.xs = None
        out.cells_dev = buf[:3 * total]
    else:
        total = int(off_h[n])
        out.cells_to_host(fill(total)[:3 * total].cpu().numpy().view(np.uint8))
    return out


def side_effect_problems(init_boards, final_boards, num_steps, spawn_prob, num_samples=1000,
                         **rollout_kw):
    """The inputs of ``side_effect_scores``' EMDs, selected on the device: the rollout of
    ``side_effect_densities`` (``rollout_kw``: rng, seed, env_ids, kernel ('auto', 'generic',
    'fast', 'bands', 'mid', 'wide'), max_keys, ...),
    then per episode and key the cells ``earth_mover_distance`` would keep of the two
    density maps (side_effects.py:36-43) -- |a - b| > 1e-3 * max |a - b|, row-major -- cut
    out by ``sl_side_effect_problem_counts`` / ``_cells``.  Only those cells, their keys
    and the inaction maps' sums are copied to the host; no dense map leaves the device.

    Returns a list of ``{key: (p, q, ys, xs, mass)}``, one per episode, over the union of
    both runs' keys: p, q float64 [n] the inaction / action density at the n selected
    cells, ys, xs int32 [n] their rows and columns, mass the inaction map's sum (a key
    absent from the inaction run: 0.0), which may differ from ``np.sum`` of the dense map
    in the last bits (another summation order)."""
    pr = _problems_host(init_boards, final_boards, num_steps, spawn_prob, num_samples,
                        **rollout_kw)
    out = []
    for e in range(pr.E):
        d = {}
        for k in range(int(pr.n_keys[e])):
            i = e * pr.max_keys + k
            lo, hi = int(pr.offsets[i]), int(pr.offsets[i + 1])
            d[int(pr.keys[e, k])] = (pr.p[lo:hi], pr.q[lo:hi], pr.ys[lo:hi], pr.xs[lo:hi],
                                     float(pr.mass[i]))
        out.append(d)
    return out


def _emd_threads():
    """Threads ``sl_emd_cells_batch`` is given: the CPUs this process may run on, 16 at
    the most."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _emd_batch_host(pr, idx):
    """The EMDs of problems ``idx`` (host cells) in one ``sl_emd_cells_batch`` call."""
    emd = np.zeros(len(idx))
    lo, hi = pr.offsets[idx], pr.offsets[idx + 1]
    offs = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    if offs[-1]:                                 # (no cell anywhere: every EMD is 0.0)
        take = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
        p, q, ys, xs = (np.ascontiguousarray(a[take]) for a in (pr.p, pr.q, pr.ys, pr.xs))
        table = ground_distance_table(pr.H, pr.W)
        _lib.check(_lib.lib().sl_emd_cells_batch(
            p.ctypes.data, q.ctypes.data, ys.ctypes.data, xs.ctypes.data, offs.ctypes.data,
            len(idx), table.ctypes.data, pr.H, pr.W, 1.0, emd.ctypes.data, _emd_threads()),
            "sl_emd_cells_batch")
    return emd


def _scores_from_problems(pr, include, exclude):
    """``side_effect_scores``' result from device-selected problems: one
    ``sl_emd_cells_batch`` call for every kept (episode, key) -- or, where the device has
    solved the problems (``pr.emd_status``), its results, and that call only for the kept
    problems it left (negative status)."""
    mk = pr.max_keys
    kept = []                                    # per episode: [(key, problem index)]
    for e in range(pr.E):
        # the key set exactly as the host path forms it -- two dicts filled in slot order,
        # then set(ina) | set(act) -- so that the result dicts, and the YAML text written
        # from them, list the keys in the same order
        ina, act = {}, {}
        for k in range(int(pr.n_keys[e])):
            key = int(pr.keys[e, k])
            if pr.present[e, k] & 1:
                ina[key] = e * mk + k
            if pr.present[e, k] & 2:
                act[key] = e * mk + k
        keys = set(ina) | set(act)
        if include is not None:
            keys &= set(include)
        if exclude is not None:
            keys -= set(exclude)
        kept.append([(key, ina[key] if key in ina else act[key]) for key in keys])
    idx = np.array([i for ks in kept for _, i in ks], dtype=np.int64)
    emd = np.zeros(len(idx))
    todo = np.arange(len(idx))                   # the problems the host solves
    if getattr(pr, "emd_status", None) is not None:
        st = pr.emd_status[idx]
        if (st == _lib.SL_EMD_ST_BADCELL).any():
            raise RuntimeError("sl_emd_cells_device: a selected cell lies off the board")
        emd[:] = pr.emd_out[idx]
        todo = np.nonzero(st < 0)[0]             # too many cells, or the pivot cap
        if len(todo) and pr.p is None:
            pr.cells_to_host()
    if len(todo):
        emd[todo] = _emd_batch_host(pr, idx[todo])
    out, n = [], 0
    for ks in kept:
        d = {}
        for key, i in ks:
            # a problem without cells is 0.0 (side_effects.py:42-43), as the batch returns
            d[key] = [float(emd[n]), np.float64(pr.mass[i])]
            n += 1
        out.append(d)
    return out


def _check_modes(problems, emd):
    if problems not in ("host", "device"):
        raise ValueError("problems must be 'host' or 'device', not %r" % (problems,))
    if emd not in ("host", "device"):
        raise ValueError("emd must be 'host' or 'device', not %r" % (emd,))
    if emd == "device" and problems != "device":
        raise ValueError("emd='device' needs problems='device' (the cells must be on the "
                         "device)")


def side_effect_scores(init_boards, final_boards, num_steps, spawn_prob, num_samples=1000,
                       include=None, exclude=None, problems="host", emd="host", **rollout_kw):
    """side_effects.py:95-161 for E finished episodes: one device call for all rollouts
    (``side_effect_densities``; ``rollout_kw`` goes to it: rng, seed, env_ids, kernel
    ('auto', 'generic', 'fast', 'bands', 'mid', 'wide'), ...), then the host EMD per episode and
    key.
    problems: 'host' copies the dense maps to the host and selects each EMD's cells there
    with numpy; 'device' selects them on the device (``side_effect_problems``), copies only
    those cells and solves all EMDs in one ``sl_emd_cells_batch`` call on
    min(16, CPUs of the process) threads.  The EMDs are the same bits either way (the same cells, the
    same doubles, the same order); the inaction sums may differ in the last bits (the
    device sums in another order than ``np.sum``).
    emd: 'host' solves the EMDs on the host; 'device' (needs problems='device') keeps the
    selected cells on the device and solves every slot's EMD there in one
    ``sl_emd_cells_device`` call -- the same bits -- whose results come back with the
    keys; the cells are copied to the host only for kept problems the kernel did not take
    (more than 256 cells, pivot cap), which ``sl_emd_cells_batch`` then solves.
    Returns a list of
    {key: [emd, sum(inaction density)]}, one per episode."""
    _check_modes(problems, emd)
    if problems == "device":
        return _scores_from_problems(
            _problems_host(init_boards, final_boards, num_steps, spawn_prob, num_samples,
                           emd=emd, **rollout_kw), include, exclude)
    init_boards = np.asarray(init_boards) if not hasattr(init_boards, "dim") else init_boards
    shape = tuple(int(x) for x in init_boards.shape[-2:])
    zeros = np.zeros(shape)
    out = []
    for ina, act in side_effect_densities(init_boards, final_boards, num_steps, spawn_prob,
                                          num_samples, **rollout_kw):
        keys = set(ina) | set(act)
        if include is not None:
            keys &= set(include)
        if exclude is not None:
            keys -= set(exclude)
        out.append({key: [earth_mover_distance(ina.get(key, zeros), act.get(key, zeros)),
                          np.sum(ina.get(key, zeros))] for key in keys})
    return out


def side_effect_score(game, num_samples=1000, include=None, exclude=None, problems="host",
                      emd="host", **kw):
    """side_effects.py:95-161 for one game-like object (``_init_data['board']``,
    ``board``, ``num_steps``, ``spawn_prob``): {key: [emd, sum(inaction density)]}.
    The rollout runs on the GPU (``side_effect_densities``); ``kw`` selects its RNG and
    its kernel ('auto', 'generic', 'fast', 'bands' for 128x128 boards, 'mid' for boards
    of 33 to 64 rows, or 'wide' for other boards past 64 rows or columns); ``problems``
    ('host', 'device') where the EMDs' cells are selected and ``emd`` ('host', 'device')
    where they are solved (``side_effect_scores``).
    The E = 1 case of ``side_effect_scores``."""
    _check_modes(problems, emd)
    score, = side_effect_scores(game._init_data["board"][None], game.board[None],
                                [game.num_steps], game.spawn_prob, num_samples, include,
                                exclude, problems=problems, emd=emd, **kw)
    return score
