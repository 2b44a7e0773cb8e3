"""The observation kernels' test cases (tests/obs_cases.py), checked without a GPU:
oracle.make_obs against views captured from the reference, and the case matrix against
the conditions it is there to reach."""
import os

import numpy as np
import pytest

import oracle
import obs_cases as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = oc.CURATED + oc.SWEEP


def fixture_states():
    d = np.load(os.path.join(GOLDEN, "obs_views.npz"))
    pos = {"board": 0, "goals": 0, "obs": 0}

    def take(k, shape):
        n = int(np.prod(shape))
        a = d[k][pos[k]:pos[k] + n].reshape(shape)
        pos[k] += n
        return a

    out = []
    for i in range(len(d["view"])):
        shape, view = tuple(int(v) for v in d["shape"][i]), tuple(int(v) for v in d["view"][i])
        chans = tuple(int(c) for c in d["channels"][i] if c >= 0)
        out.append({"board": take("board", shape), "goals": take("goals", shape),
                    "ax": int(d["agent_loc"][i][0]), "ay": int(d["agent_loc"][i][1]),
                    "exits": [(int(y), int(x)) for y, x in d["exits"][i][:int(d["exit_count"][i])]],
                    "view": view, "channels": chans or None,
                    "remove_white": bool(d["remove_white"][i]),
                    "obs": take("obs", view + ((len(chans),) if chans else ()))})
    assert all(pos[k] == len(d[k]) for k in pos)
    return out


def obs_of(s, exits=None):
    return oracle.make_obs(s["board"], s["goals"], s["ax"], s["ay"],
                           s["exits"] if exits is None else exits, s["view"], s["channels"],
                           s["remove_white"])


def test_make_obs_equals_reference_fixture():
    """oracle.make_obs reproduces every view of obs_views.npz, which make_golden.py (gen_obs)
    captured from the reference's SafeLifeEnv.get_obs.  The reference raised on none of
    the 40 states, so none is left out."""
    sts = fixture_states()
    assert len(sts) == len(oc.FIXTURE_SPECS) == 40
    for i, s in enumerate(sts):
        got = obs_of(s)
        assert got.shape == s["obs"].shape, i
        assert np.array_equal(got.astype(np.int64), s["obs"].astype(np.int64)), i


def test_fixture_holds_the_states_it_is_there_for():
    sts = fixture_states()
    shapes = {(s["board"].shape, s["view"]) for s in sts}
    assert ((2, 2), (9, 9)) in shapes and ((3, 5), (1, 64)) in shapes
    assert {(9, 70), (33, 40)} <= {s["board"].shape for s in sts}
    assert all(s["board"].shape[0] <= 16 and s["board"].shape[1] <= 16 for s in sts
               if s["board"].shape not in ((9, 70), (33, 40)))
    views = {s["view"] for s in sts}
    assert (1, 1) in views
    assert any(h == 1 and w > 1 for h, w in views) and any(w == 1 and h > 1 for h, w in views)
    assert any(h % 2 == 0 and w % 2 == 0 for h, w in views)
    assert {0, 1, 8} <= {len(s["exits"]) for s in sts}
    assert {True, False} == {s["remove_white"] for s in sts if white_goal(s)}
    assert any(carries(s) for s in sts)
    stacked = set()
    corners = set()
    half_h = half_w = False
    for s in sts:
        (H, W), (vh, vw) = s["board"].shape, s["view"]
        tgt, clipped = oc.exit_targets(H, W, vh, vw, s["ay"], s["ax"])
        for n in stacked_exits(s):
            stacked.add(n)
        for y, x in s["exits"]:
            if tgt[y, x] in (0, vw - 1, (vh - 1) * vw, vh * vw - 1) and vh > 1 and vw > 1:
                corners.add((0, vw - 1, (vh - 1) * vw, vh * vw - 1).index(tgt[y, x]))
            half_h |= H % 2 == 0 and (y - s["ay"]) % H == H // 2
            half_w |= W % 2 == 0 and (x - s["ax"]) % W == W // 2
    assert {2, 3} <= stacked
    assert corners == {0, 1, 2, 3}
    assert half_h and half_w


# ------------------------------------------------------------------ what a state holds
def white_goal(s):
    return bool(((s["goals"] & oc.RAINBOW) == oc.RAINBOW).any())


def carries(s):
    """Does board + (goals & colours) << 3 carry out of bit 15 in some cell?"""
    g = (s["goals"] & oc.RAINBOW).astype(np.int64)
    if s["remove_white"]:
        g = g * (g != oc.RAINBOW)
    return bool(((s["board"].astype(np.int64) + (g << 3)) >> 16).any())


def stacked_exits(s):
    """Sizes of the groups of exits that clip onto one target while holding different
    values, found on the oracle: reversing the group's order changes the view."""
    (H, W), (vh, vw) = s["board"].shape, s["view"]
    tgt, clipped = oc.exit_targets(H, W, vh, vw, s["ay"], s["ax"])
    groups = {}
    for k, (y, x) in enumerate(s["exits"]):
        if clipped[y, x]:
            groups.setdefault(int(tgt[y, x]), []).append(k)
    sizes = []
    for ks in groups.values():
        if len(ks) < 2:
            continue
        order = list(range(len(s["exits"])))
        for a, b in zip(ks, reversed(ks)):
            order[a] = b
        if not np.array_equal(obs_of(s), obs_of(s, [s["exits"][k] for k in order])):
            sizes.append(len(ks))
    return sizes


def env_states(case):
    st = oc.make_states(case)
    for b in range(case.B):
        yield {"board": st["board"][b], "goals": st["goals"][b], "ax": int(st["agent_x"][b]),
               "ay": int(st["agent_y"][b]), "exits": st["exits"][b], "view": case.view,
               "channels": None, "remove_white": case.remove_white}


# --------------------------------------------------------------- the matrix's coverage
def test_case_names_and_batches():
    assert len({c.name for c in ALL}) == len(ALL)
    assert 180 <= len(oc.SWEEP) <= 220
    for c in ALL:
        assert c.B >= 5 and c.B % 4 != 0
        assert 1 <= c.nv <= oc.MAX_CELLS
    for c in oc.SWEEP:
        assert c.B == 5 and max(c.shape) <= 40 and c.nv <= oc.SWEEP_MAX_CELLS
        assert set(c.view) <= set(oc.SWEEP_SIDES)
        assert 1 <= len(c.channels or (0,)) <= 16


def test_curated_views_boards_lists_and_modes():
    assert oc.VIEWS[-1][0] * oc.VIEWS[-1][1] == oc.MAX_CELLS
    assert {(65, 63), (64, 64), (64, 65)} <= set(oc.VIEWS)
    assert 65 * 63 == oc.WAVE_MAX_CELLS - 1 and 64 * 64 == oc.WAVE_MAX_CELLS
    for view in oc.VIEWS:
        cs = [c for c in oc.CURATED if c.view == view]
        assert len({c.shape for c in cs}) >= 2, view
        assert {(c.mode, c.offset) for c in cs} >= {(m, o) for m in oc.MODES
                                                    for o in (False, True)}, view
    assert {c.shape for c in oc.CURATED} == set(oc.BOARDS)
    for chans in oc.CHANNEL_LISTS:
        for mode in oc.MODES[1:]:
            assert {c.offset for c in oc.CURATED if c.channels == chans and c.mode == mode} \
                == {False, True}, (chans, mode)
    assert any(len(set(ch)) < len(ch) for ch in oc.CHANNEL_LISTS)
    assert tuple(range(15, -1, -1)) in oc.CHANNEL_LISTS


def test_every_kernel_in_every_mode_it_serves():
    reached = {(c.kernel, c.mode) for c in ALL}
    want = {("wave-packed", "packed"), ("fallback", "packed")}
    want |= {(k, m) for k in ("chunk", "fallback") for m in oc.MODES[1:]}
    assert reached == want
    for pool in (oc.CURATED, oc.SWEEP):     # each list alone reaches the three kernels
        assert {c.kernel for c in pool} == {"wave-packed", "chunk", "fallback"}
    # the fallback is reached both ways: a large view, and an output off 16 bytes
    fb = [c for c in ALL if c.kernel == "fallback" and c.mode != "packed"]
    assert any(c.nv > oc.WAVE_MAX_CELLS and not c.offset for c in fb)
    assert any(c.nv <= oc.WAVE_MAX_CELLS and c.offset for c in fb)
    # the wave kernels at their last size, the fallback at the first past it
    for mode in oc.MODES:
        k = "wave-packed" if mode == "packed" else "chunk"
        assert any(c.nv == oc.WAVE_MAX_CELLS and c.kernel == k and c.mode == mode for c in ALL)
        assert any(c.nv == 64 * 65 and c.kernel == "fallback" and c.mode == mode
                   and not c.offset for c in ALL)


@pytest.mark.parametrize("esz", [1, 2, 4])
def test_chunk_kernel_heads_tails_and_short_envs(esz):
    cs = [c for c in ALL if c.kernel == "chunk" and c.esz == esz]
    parts = [(c, c.env_parts(b)) for c in cs for b in range(c.B)]
    # a head, whole chunks and a tail; and neither head nor tail
    assert any(h and n and t for _, (h, n, t, _) in parts)
    assert any(not h and n and not t for _, (h, n, t, _) in parts)
    # next to whole chunks, heads and tails of every length an element size allows
    assert {h for _, (h, n, _, _) in parts if n} == set(range(0, 16, esz))
    assert {t for _, (_, n, t, _) in parts if n} == set(range(0, 16, esz))
    short = [(c, p) for c, p in parts if c.env_bytes < 16]
    assert any(not cross for _, (_, _, _, cross) in short)
    assert any(cross and h and t for _, (h, _, t, cross) in short)
    # the gather takes a chunk's 16 / esz element bits from up to that many masks
    assert any(c.nch == 1 and c.env_bytes >= 64 for c in cs)
    assert any(c.nch == 16 for c in cs) and any(15 in c.channels for c in cs)


def test_view_sizes_widths_and_wraps():
    for pool in (ALL, [c for c in ALL if c.kernel == "wave-packed"],
                 [c for c in ALL if c.kernel == "chunk"]):
        assert any(c.nv < 64 for c in pool)
        assert any(c.nv > 64 and c.nv % 64 for c in pool)
        assert any(c.nv > 512 for c in pool)
        vws = [c.view[1] for c in pool]
        assert 1 in vws and 64 in vws
        assert any(2 <= w <= 63 for w in vws) and any(65 <= w <= 128 for w in vws)
        assert any(w > 128 for w in vws)
        # 64 is no multiple of vw: the per-lane column step carries into the row
        assert any(64 % w and w < 64 for w in vws)
    assert any(c.view[0] >= 3 * c.shape[0] for c in ALL)
    assert any(c.view[1] >= 3 * c.shape[1] for c in ALL)
    assert any(c.view[0] % 2 == 0 and c.view[1] % 2 == 0 for c in ALL)


def test_states_hold_the_exits_and_values_they_claim():
    """By the oracle, over the committed seeds of the curated cases and the sweep."""
    seen = {k: False for k in ("stack2", "stack3", "half_h", "half_w", "none", "eight",
                               "inside", "carry", "white_kept", "white_removed")}
    for c in ALL:
        if c.nv > 1100 or c.shape[0] * c.shape[1] > 4096:   # (the small cases suffice)
            continue
        (H, W), (vh, vw) = c.shape, c.view
        for s in env_states(c):
            n = len(s["exits"])
            seen["none"] |= n == 0
            seen["eight"] |= n == 8
            sizes = stacked_exits(s) if n >= 2 else []
            seen["stack2"] |= 2 in sizes
            seen["stack3"] |= 3 in sizes
            tgt, clipped = oc.exit_targets(H, W, vh, vw, s["ay"], s["ax"])
            for y, x in s["exits"]:
                seen["half_h"] |= H % 2 == 0 and (y - s["ay"]) % H == H // 2
                seen["half_w"] |= W % 2 == 0 and (x - s["ax"]) % W == W // 2
                seen["inside"] |= not clipped[y, x]
            seen["carry"] |= carries(s)
            seen["white_removed" if c.remove_white else "white_kept"] |= white_goal(s)
    assert all(seen.values()), seen
