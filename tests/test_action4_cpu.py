"""action4 (csrc/sl_action4.h), the agent's action as one straight-line function of four
cells, against OracleEnv._execute_action.

A stand-alone host program is built from the header with the system compiler (the header is
plain C++).  It reads one case per line and prints action4's result.  The oracle runs the same
cases on a small torus: the agent's cell (c0), the cell in front (c1), behind (c2) and two
ahead (c3) are set, the action executed, and reward, game_over, agent position, orientation
and the four cells compared.

Cases: all nine actions x game_over x can_exit x (can_toggle_powers, can_toggle_colors) in
{(0,0), (1,1), (1,0)} x c0 in the agent values of the c3 / c4 pools (one: 0x7A; and the agent
coloured by an xor toggle) x c1, c2, c3 from CELLS: empty, wall, the closed and the open exit,
the crate 0x8014, a pushable-only and a pullable-only cell, living life in the pools' colours
(red 0x209, green 0x409), frozen life 0x411, a destructible dead cell.  can_exit is an input
of the function (the caller evaluates can_exit_now), so the oracle's _can_exit is set to it.

The branches of act_core are counted from the oracle's side alone (its board before and
after), each at least once.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "safelife-k2_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

EXIT, PUSHABLE, PULLABLE, DESTR = 0x0100, 0x0004, 0x8000, 0x0008
CELLS = [0x0000, 0x0010, 0x0110, 0x0310, 0x8014, 0x0014, 0x8010, 0x0209, 0x0409, 0x0411, 0x0008]
AGENTS = [0x007A, 0x047A]
TOGGLES = [(0, 0), (1, 1), (1, 0)]
Y0, X0, S = 2, 3, 7             # the agent's cell on an S x S torus (S >= 5: four distinct cells)

MAIN = r"""
#include <cstdio>
#include "sl_action4.h"
int main() {
    int a, go, can, ctp, ctc;
    unsigned c0, c1, c2, c3;
    while (std::scanf("%d %d %d %d %d %x %x %x %x", &a, &go, &can, &ctp, &ctc, &c0, &c1, &c2,
                      &c3) == 9) {
        const sl::act4::Result r = sl::act4::action4(a, go, can != 0, ctp, ctc, c0, c1, c2, c3);
        std::printf("%d %d %d %d %d %d %u %u %u %u %u\n", r.reward, r.game_over, r.moved, r.orient,
                    r.store_orient, r.store_agent, r.n[0], r.n[1], r.n[2], r.n[3], r.changed);
    }
    return 0;
}
"""


def _cases():
    return list(itertools.product(range(9), (0, 1), (0, 1), TOGGLES, AGENTS, CELLS, CELLS, CELLS))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """action4 over _cases(): one row of eleven integers per case."""
    d = tmp_path_factory.mktemp("action4")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = str(d / "action4")
    subprocess.check_call([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src),
                           "-o", exe])
    text = "".join("%d %d %d %d %d %x %x %x %x\n" % (a, go, can, t[0], t[1], c0, c1, c2, c3)
                   for a, go, can, t, c0, c1, c2, c3 in _cases())
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
    return np.array(out.split(), dtype=np.int64).reshape(-1, 11)


def _cells_of(orient):
    """(y, x) of the agent's cell, the front, the one behind and the one two ahead."""
    dy, dx = ((-1, 0), (0, 1), (1, 0), (0, -1))[orient]
    return [((Y0 + k * dy) % S, (X0 + k * dx) % S) for k in (0, 1, -1, 2)]


def test_against_the_oracle(results):
    cases = _cases()
    assert len(results) == len(cases)
    env = oracle.OracleEnv(None)
    env.goals = np.zeros((S, S), np.uint16)
    seen = dict.fromkeys(("empty front", "open exit", "closed exit", "push into empty",
                          "push into exit", "blocked", "pull", "no pull without a move",
                          "toggle create", "toggle destroy", "toggle xor", "game over", "null"), 0)
    can = [False]
    env._can_exit = lambda: can[0]
    for (a, go, ce, t, c0, c1, c2, c3), r in zip(cases, results):
        # orientation before: anything but what the action sets, so a store shows
        orient = (a - 1) & 3
        before = (orient + 1) & 3
        yx = _cells_of(orient)
        env.board = b = np.zeros((S, S), np.uint16)
        for (y, x), v in zip(yx, (c0, c1, c2, c3)):
            b[y, x] = v
        env.agent_loc = (X0, Y0)
        env.orientation = before
        env.game_over = bool(go)
        env.can_toggle_powers, env.can_toggle_colors = t
        can[0] = bool(ce)
        reward = env._execute_action(oracle.ACTIONS[a])
        after = [int(b[y, x]) for y, x in yx]
        moved = env.agent_loc == (yx[1][1], yx[1][0])
        c = (a, go, ce, t, hex(c0), hex(c1), hex(c2), hex(c3))

        assert r[0] == reward, c
        assert bool(r[1]) == bool(env.game_over), c
        assert bool(r[2]) == moved, c
        assert moved or env.agent_loc == (X0, Y0), c
        # the orientation the kernel stores, where it stores one
        assert (r[3] if r[4] else before) == env.orientation, c
        assert r[5] == (1 if (not go and 1 <= a <= 4) else 0), c
        assert [int(v) for v in r[6:10]] == after, c
        assert r[10] == sum(1 << k for k in range(4) if after[k] != (c0, c1, c2, c3)[k]), c
        # no other cell of the board is touched
        assert int(np.count_nonzero(b)) == sum(v != 0 for v in after), c

        # act_core's branches, from the oracle's board alone
        if go:
            seen["game over"] += 1
        elif a == 0:
            seen["null"] += 1
        elif a <= 4:
            if c1 == 0:
                seen["empty front"] += moved
            elif reward:
                seen["open exit"] += 1
            elif moved and after[3] == c1 and c3 == 0:
                seen["push into empty"] += 1
            elif moved and (c3 & EXIT) and after[3] == c3:
                seen["push into exit"] += 1
            elif not moved:
                seen["closed exit" if c1 & EXIT else "blocked"] += 1
            if moved and (c2 & PULLABLE):
                seen["pull"] += after[0] == c2 and after[2] == 0
            if not moved and (c2 & PULLABLE):
                seen["no pull without a move"] += after[2] == c2
        else:
            if c1 == 0:
                seen["toggle create"] += after[1] == (0x0009 | (c0 & 0x0E00))
            elif c1 & DESTR:
                seen["toggle destroy"] += after[1] == 0
            else:
                seen["toggle xor"] += after[0] != c0
    print(seen)
    assert all(n >= 1 for n in seen.values()), seen
