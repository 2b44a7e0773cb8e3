"""The stand-alone observation kernels behind sl_env_obs (k_env_obs_packed,
k_env_obs_channels<1|2|4>, k_env_obs; sl_env.hip, sl_obs.h) against oracle.make_obs over
the case matrix of tests/obs_cases.py: explicit states loaded with set_state, one
observe(), every byte compared.  tests/test_obs_cases_cpu.py pins make_obs to the
reference and checks what the cases reach."""
import numpy as np
import pytest

import oracle  # noqa: F401  (obs_cases imports it; kept visible here as the checker)
import obs_cases as oc

pytestmark = pytest.mark.gpu

FILL = 0xA5                 # every byte of an output buffer before the kernel writes


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def blank_level(shape):
    from safelife_amd.cell_types import CellTypes as CT
    board = np.zeros(shape, np.uint16)
    board[0, 0] = CT.player
    return {"board": board, "goals": np.zeros(shape, np.uint16), "agent_loc": np.array([0, 0])}


def raw_bits(torch, t):
    """A tensor's elements as unsigned integers (numpy int64)."""
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    if t.dtype == torch.bfloat16:
        t = t.view(torch.uint16)
    return t.cpu().numpy().astype(np.int64)


def expected_bits(case, st):
    want = oc.expected(case, st)
    return want if case.mode == "packed" else want * oc.ONE[case.mode]


def out_buffer(torch, dev, venv, case):
    """An output like venv.obs inside a buffer of FILL bytes: at the buffer's start
    (16-byte aligned) or one element in, and one guard element after it."""
    n, esz = venv.obs.numel(), venv.obs.element_size()
    assert esz == case.esz
    raw = torch.full(((n + 2) * esz,), FILL, dtype=torch.uint8, device=dev).view(venv.obs.dtype)
    lo = 1 if case.offset else 0
    out = raw[lo:lo + n].view(venv.obs.shape)
    assert out.data_ptr() % 16 == case.out_shift
    return raw, out, lo


def run_case(torch, dev, case):
    """Observe the case's states; returns None, or what differs."""
    from safelife_amd import SafeLifeVecEnv, LevelPool, _lib
    venv = SafeLifeVecEnv(LevelPool.from_levels([blank_level(case.shape)]), case.B, dev,
                          view_shape=case.view, output_channels=case.channels,
                          obs_dtype="uint16" if case.mode == "packed" else case.mode,
                          remove_white_goals=case.remove_white, compute_obs=False)
    st = oc.make_states(case)
    venv.set_state(st["board"], st["goals"], st["board"],
                   **{k: st[k] for k in ("agent_x", "agent_y", "exit_count", "exit_y", "exit_x")})
    raw, out, lo = out_buffer(torch, dev, venv, case)
    try:
        got = venv.observe(out=out)
    except RuntimeError as e:
        # only a view whose staging array outgrows what a launch may ask for is refused
        assert "code %d" % _lib.SL_ETOOBIG in str(e) and case.kernel == "fallback" \
            and case.nv * 2 > 65536, (case, e)
        return None
    torch.cuda.synchronize()
    # the path taken was observe on the uint16 board: nothing stepped, and where a batch
    # keeps bit planes (64x64, 128x128) set_state left every env's stale
    assert got is out and venv._step_index == 0 and venv._last_step is None
    assert venv._last_mode is None
    assert int(venv.planes_ok.abs().sum().item()) == 0
    have, want = raw_bits(torch, out), expected_bits(case, st)
    if have.shape != want.shape:
        return "%s: shape %s, expected %s" % (case, have.shape, want.shape)
    if not np.array_equal(have, want):
        bad = np.argwhere(have != want)
        return "%s (%s): %d of %d elements differ, first at %s: %#x, expected %#x" % (
            case, case.kernel, len(bad), have.size, tuple(bad[0]), have[tuple(bad[0])],
            want[tuple(bad[0])])
    guard = raw_bits(torch, raw)
    fill = int.from_bytes(bytes([FILL]) * case.esz, "little")
    if not (guard[:lo] == fill).all() or not (guard[lo + out.numel():] == fill).all():
        return "%s (%s): wrote outside its output" % (case, case.kernel)
    return None


@pytest.mark.parametrize("case", oc.CURATED, ids=[c.name for c in oc.CURATED])
def test_observe_vs_oracle(torch_dev, case):
    torch, dev = torch_dev
    assert run_case(torch, dev, case) is None


def test_observe_sweep_vs_oracle(torch_dev):
    torch, dev = torch_dev
    bad = [r for r in (run_case(torch, dev, c) for c in oc.SWEEP) if r is not None]
    assert not bad, "%d of %d cases: %s" % (len(bad), len(oc.SWEEP), "; ".join(bad[:5]))


def _curated(shape, mode):
    return next(c for c in oc.CURATED if c.shape == shape and c.mode == mode
                and 64 < c.nv <= 4096 and not c.offset)


@pytest.mark.parametrize("shape,mode", [((25, 25), "packed"), ((33, 40), "uint16"),
                                        ((9, 70), "packed")])
def test_single_env_get_obs_vs_oracle(torch_dev, shape, mode):
    """The B = 1 drop-in: SafeLifeEnv.get_obs with a board, goals and an agent cell of the
    caller's (its own sl_env_obs call, on a slice of the env's state), and without."""
    torch, dev = torch_dev
    from safelife_amd.env import SafeLifeEnv
    case = _curated(shape, mode)
    st = oc.make_states(case)
    env = SafeLifeEnv(iter([blank_level(case.shape)]), device=dev, rng="philox", seed=1,
                      view_shape=case.view, output_channels=case.channels,
                      remove_white_goals=case.remove_white)
    env.reset()
    want = oc.expected(case, st)
    for b in range(case.B):
        one = {k: st[k][b:b + 1] for k in ("agent_x", "agent_y", "exit_count", "exit_y", "exit_x")}
        # the exits are the game's; board, goals and agent come with the call
        blank = np.zeros((1,) + case.shape, np.uint16)
        env._venv.set_state(blank, blank, blank, **dict(one, agent_x=[0], agent_y=[0]))
        got = env.get_obs(board=st["board"][b], goals=st["goals"][b],
                          agent_loc=(int(st["agent_x"][b]), int(st["agent_y"][b])))
        assert got.shape == want[b].shape
        assert np.array_equal(got.astype(np.int64), want[b]), (case, b)
        # and the game's own state
        env._venv.set_state(st["board"][b:b + 1], st["goals"][b:b + 1], st["board"][b:b + 1], **one)
        assert np.array_equal(env.get_obs().astype(np.int64), want[b]), (case, b)
