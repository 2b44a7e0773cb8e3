// sl_action4.h -- the agent's action (execute_action / move_agent, safelife_game.py:308-393)
// as one straight-line function of the four cells it can read: the agent's (c0), the one in
// front (c1), the one behind (c2) and the one two ahead (c3).  Same semantics as act_core
// (sl_action.h), tests in the same order, for a board on which the four cells are distinct
// (a torus of at least five rows and columns); no loops, no overlay, no index search.
// Plain C++ (no HIP builtins): a host program includes it as it is
// (tests/test_action4_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SL_ACT4_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SL_ACT4_FN inline
#endif

namespace sl {
namespace act4 {

// cell bits (sl_device.h's, restated so the header stands alone)
constexpr uint32_t kAlive = 0x0001, kPushable = 0x0004, kDestr = 0x0008, kPreserve = 0x0020;
constexpr uint32_t kInhibit = 0x0040, kSpawn = 0x0080, kExit = 0x0100, kColors = 0x0E00;
constexpr uint32_t kPullable = 0x8000;
constexpr uint32_t kLife = kAlive | kDestr;
constexpr uint32_t kPowers = kAlive | kInhibit | kPreserve | kSpawn;

struct Result {
    int reward;          // 1: the agent walked into an open exit
    int game_over;       // after the action
    int moved;           // the agent is on the front cell now
    int orient;          // the orientation to store ...
    int store_orient;    // ... when the action runs at all
    int store_agent;     // a move action (moved or not): act_core stores the position
    uint32_t n[4];       // the four cells after the action
    uint32_t changed;    // bit k: n[k] differs from the cell before
};

// a: 0..8 (safelife_env.py:61-71; 0 and anything above 8 do nothing).  can_exit: the
// caller's can_exit_now.  ctp, ctc: the toggle copies powers / colours.
SL_ACT4_FN Result action4(int a, int game_over, bool can_exit, int ctp, int ctc, uint32_t c0,
                          uint32_t c1, uint32_t c2, uint32_t c3) {
    const bool active = !game_over && a >= 1 && a <= 8;
    const bool mv = active && a <= 4, tg = active && a > 4;
    // move_agent: empty front; open exit; push into empty; push into exit; else blocked
    const bool empty = c1 == 0;
    const bool enter = !empty && (c1 & kExit) && can_exit;
    const bool push = !empty && !enter && (c1 & kPushable);
    const bool push_empty = push && c3 == 0;
    const bool push_exit = push && c3 != 0 && (c3 & kExit);      // the pushed cell is gone
    const bool moved = mv && (empty || push_empty || push_exit);
    const bool pull = moved && (c2 & kPullable);                  // only after a move
    // toggle: create, destroy, else xor the agent with the cell's powers / colours
    const bool create = tg && c1 == 0;
    const bool destroy = tg && c1 != 0 && (c1 & kDestr);
    const bool txor = tg && !create && !destroy;
    const uint32_t tbits = (ctp ? kPowers : 0u) | (ctc ? kColors : 0u);

    Result r;
    r.reward = (mv && enter) ? 1 : 0;
    r.game_over = r.reward ? 1 : game_over;
    r.moved = moved ? 1 : 0;
    r.orient = (a - 1) & 3;
    r.store_orient = active ? 1 : 0;
    r.store_agent = mv ? 1 : 0;
    r.n[0] = moved ? (pull ? c2 : 0u) : (txor ? c0 ^ (c1 & tbits) : c0);
    r.n[1] = moved ? c0 : (create ? (kLife | (c0 & kColors)) : (destroy ? 0u : c1));
    r.n[2] = pull ? 0u : c2;
    r.n[3] = (mv && push_empty) ? c1 : c3;
    r.changed = (r.n[0] != c0 ? 1u : 0u) | (r.n[1] != c1 ? 2u : 0u) | (r.n[2] != c2 ? 4u : 0u) |
                (r.n[3] != c3 ? 8u : 0u);
    return r;
}

}  // namespace act4
}  // namespace sl
