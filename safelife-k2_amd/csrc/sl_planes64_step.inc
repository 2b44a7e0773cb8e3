// sl_planes64_step.inc -- one plane-mode env-step of env blockIdx.x: the body of the
// kernels k_env_step_bits64_planes and k_env_planes64_chan (sl_bits.hip), included inside
// each, which sets DM, the derived planes the instance is compiled for (PlaneSlots).
// (Text, not a force-inlined function: as a function templated on <K16, OBS> and
// called from thin kernels, the same statements left k_env_step_bits64_planes<0x877F, 0>
// with 3692 spilled VGPRs and 3112 B of scratch at its 96-register budget, and moved the
// run-time-mask instances by two registers; included, the six older kernels compile to
// the instructions they had.)  In scope where it is included: the template parameters K16
// (kept planes; 0: from board_zero) and OBS (k_env_step_bits64's: 0 none, 1 packed views
// by write_obs, 2-4 channel views by write_obs_channels<obs_esz(OBS)>), the constant GRAY
// (k_env_planes64_gray's: sl_env_state.goals_gray holds, every goal cell black or white --
// the scores read no goal colour, the packed views one plane; OBS <= 1), the kernel's
// argument `StepKArgs ka`, the wave's buffer `u32 stage[N * N / 2]` in LDS, and `vm`, the
// view's channel masks in LDS (uint16_t[kFusedChanCells]; unused when OBS < 2), and the
// constant W6 (k_env_planes64_w6's: `stage` is 6 KiB, not 8 -- the pool's start-plane rows
// are packed, a uint16 board is staged in two passes of 32 rows, and the scores read the
// start planes one column word at a time; OBS == 0), and the constant SPLIT_EPI
// (k_env_planes64_s6's: the wave ends after its stores with the env's hand-over record, and
// k_env_epilogue_reset64 runs the epilogue and the resets, one lane per env).
// With views, the goal colours are added into planes 12-14 (a bit-sliced adder, exact
// whatever the board's bits), ONE transpose puts the view-form rows into the buffer.
    const sl_env_state &st = ka.st;
    const StepArgs &a = ka.a;
    const FastExtra &fx = ka.fx;
    const int64_t b = blockIdx.x;          // one wave per env
    const int lane = threadIdx.x;
    lds_u32 *buf = (lds_u32 *)&stage[0];
    const PlaneSlots<K16, DM> ps = PlaneSlots<K16, DM>::of(st.board_zero, st.agent_planes,
                                                           st.derived_planes);
    // what the buffer holds at one time: the stored plane words, the pool's start-plane
    // rows, or (W6) half a uint16 board
    constexpr int kStageDw = (int)(sizeof(stage) / sizeof(u32));
    static_assert(!W6 || (PlaneSlots<K16, DM>::kFixed && OBS == 0), "W6: fixed planes, no views");
    // the stored words: held, not the agent's, not derived (DM 0x8100: twelve, 3 KiB; the
    // stored-16 twins: sixteen, 4 KiB)
    constexpr int kStoredWords =
        2 * __builtin_popcount(K16 & ~kAgentC3 & ~(u32)(DM > 0 ? DM : 0) & 0xFFFFu);
    static_assert(K16 != kKeepC3 || kStoredWords == (DM ? 12 : 16), "three DMA groups, or four");
    static_assert(!W6 || kStoredWords * 64 <= kStageDw, "the stored plane words fit the buffer");
    static_assert(pool_rows_dwords(K16 ? K16 : 0xFFFFu, W6) <= kStageDw,
                  "the pool's start-plane rows fit the buffer");
    static_assert(kStageDw >= (W6 ? N * N / 4 : N * N / 2), "a board, or half of one (W6)");
    Pre pre;
    // GRAY: no colour plane for the scores (rows black and white of the point table are
    // equal, neither counts as possible or as a blue goal: they score as black, 0); the
    // views add the colours to the board's, so they load one plane for the three -- none
    // where white goals are removed, which leaves only black ones
    const bool gray_blank = GRAY && (!OBS || fx.obs_rw != 0);
    if (!GRAY) issue_pre(st, ka.actions, b, lane, pre);
    else if (gray_blank) issue_pre<0>(st, ka.actions, b, lane, pre);
    else issue_pre<1>(st, ka.actions, b, lane, pre);
    // the board's planes, speculatively: an env whose planes do not hold its board (the
    // first step after a host write or a step in another mode) reloads its rows below
    dma_planes(st.planes + b * 4096, ps, buf, lane);
    const int64_t off = b * (int64_t)(N * N);
    const int lane_off = (lane & 1) * 1024 + (lane >> 1);     // dwords: row 32h, column pair j
    u32 *gg = reinterpret_cast<u32 *>(st.goals + off) + lane_off;
    u32 *mg = st.planes + b * 4096 + 2048 + lane;
    u32 *bp = st.planes + b * 4096 + lane;
    const u32 V = pre.V;
    const int pok_all = rec(V, R_POK);
    const bool pin = (pok_all & SL_POK_BOARD_PLANES) != 0;
    u32 gcol[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gcol[k][0] = pre.g[k][0];
        gcol[k][1] = pre.g[k][1];
    }
    const int pok = pok_all & kPokGoalsSkip;

    const SpawnCtx sc = spawn_ctx(a, b, rec(V, R_SPAWN));
    const StreamSrc ssrc{a.draws, a.n_draws, nullptr, a.draw_mask, a.draw_bits};

    // ---- goals: the mirror is half 1 of the planes; their planes_ok bits after this
    // step go out with the board's below
    int gok = pok;
    if ((pok & kPokGoalsSkip) != kPokGoalsSkip)
        gok = goals_step64<true, SPAWN_PHILOX>(gg, mg, pok, lane, sc, ssrc, 0, gcol);
    __builtin_amdgcn_sched_barrier(0);

    int roll = -1;
    if (fx.pool.K > 0 && fx.pool.board_planes && st.start_roll) roll = rec(V, R_ROLL);
    // The action reads four cells -- the agent's, the one in front, the one behind, the one
    // two ahead (sl_action4.h) -- and which four is in the record: their indices, the exits
    // among them and can_exit are worked out while the planes are in flight.  (ACT4: the
    // instances with compile-time plane masks.  Those with run-time masks, K16 == 0, keep
    // act_core on a nine-cell gather: with this form k_env_planes64_chan<0, *> and
    // k_env_step_bits64_planes<0, 1> gained 68 B of scratch per lane.)
    constexpr bool ACT4 = K16 != 0;
    static_assert(N >= 5 && (N & (N - 1)) == 0, "the four cells are distinct; wrapped by mask");
    const int act = rec(V, R_ACT), go0 = rec(V, R_GO);
    const int ay0 = rec(V, R_AY), ax0 = rec(V, R_AX);
    int eidx[4] = {0, 0, 0, 0};     // the edited cells' flat indices
    int cell_i = 0;                 // (ACT4) this lane's cell: cell lane & 3
    u32 exit_hits = 0u;             // (ACT4) bit k + 4 e: cell k is exit e of the record's list
    bool can_exit0 = false;
    if (ACT4) {
        const int orient = (act - 1) & 3;
        const int fdx = orient == 1 ? 1 : (orient == 3 ? -1 : 0);
        const int fdy = orient == 0 ? -1 : (orient == 2 ? 1 : 0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int d = k == 2 ? -1 : (k == 3 ? 2 : k);
            eidx[k] = ((ay0 + d * fdy) & (N - 1)) * N + ((ax0 + d * fdx) & (N - 1));
        }
        cell_i = (lane & 2) ? ((lane & 1) ? eidx[3] : eidx[2])
                            : ((lane & 1) ? eidx[1] : eidx[0]);
        // lane k + 4 e compares cell k with exit e (the derived exit plane has no words to
        // gather the bit from)
        if (ps.drv16() & 0x0100u) {
            const int e = (lane >> 2) & 7;
            const int sh = 16 * (e & 1);
            const int ey = (int)(int16_t)(
                __builtin_amdgcn_ds_bpermute(4 * (R_EY + (e >> 1)), (int)V) >> sh);
            const int ex = (int)(int16_t)(
                __builtin_amdgcn_ds_bpermute(4 * (R_EX + (e >> 1)), (int)V) >> sh);
            const int n = min(rec(V, R_EXC), SL_MAX_EXITS);
            exit_hits = (u32)__ballot(lane < 32 && e < n && ey * N + ex == cell_i);
        }
        can_exit0 = can_exit_now(rec_f64(V, R_MP), rec(V, R_SCORE), rec(V, R_BASE),
                                 rec(V, R_POSS));
    }
    wait_vm();
    if (!pin) {
        // a step into plane mode: the uint16 board instead, transposed and put into the
        // buffer in the planes' layout, so everything below reads planes
        if (!W6) {
            dma_board(st.board + off, buf, lane);
            wait_vm();
        }
        u32 R[32];
        if (W6) board_pairs_halves(st.board + off, buf, lane, R);
        else read_pairs(buf, lane, R);
        transpose32(R);
#pragma unroll
        for (int q = 0; q < 32; q++)
            if (ps.stored(q)) buf[ps.pos(q) * 64 + lane] = R[q];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    int act_reward = 0, go1 = go0, ax1 = ax0, ay1 = ay0;    // ..1: after the action
    u32 echg = 0u;                  // bit k: cell eidx[k] becomes eval[k]
    u32 eval[4];
    if (ACT4) {
        // wave-uniform: every lane reads its cell's stored planes (four addresses,
        // broadcast), lanes 0-3 hand the four cells to scalars, action4 decides; four fixed
        // slots of edits, in any order (the cells are distinct)
        const u32 cell_v = lds_plane_cell_stored(buf, ps, cell_i);
        u32 cell[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cell[k] = (u32)__builtin_amdgcn_readlane((int)cell_v, k);
            if ((ps.drv16() & 0x0100u) && (exit_hits & (0x11111111u << k))) cell[k] |= EXIT;
        }
        // (the agent planes' bits are in the agent's cell, and in no other)
        cell[0] |= ps.agent16();
        const act4::Result ar = act4::action4(act, go0, can_exit0, ka.ctp, ka.ctc, cell[0],
                                              cell[1], cell[2], cell[3]);
        act_reward = ar.reward;
        go1 = ar.game_over;
        if (ar.moved) {
            ax1 = eidx[1] & (N - 1);
            ay1 = eidx[1] / N;
        }
        if (lane == 0) {
            if (ar.store_orient) st.orientation[b] = ar.orient;
            if (ar.reward) st.game_over[b] = 1;
            if (ar.store_agent) {
                st.agent_x[b] = ax1;
                st.agent_y[b] = ay1;
            }
        }
        echg = ar.changed;
#pragma unroll
        for (int k = 0; k < 4; k++) eval[k] = ar.n[k];
    } else {
        // lane 0, on the cells round the agent gathered from the staged planes (kept copy
        // of step_env's prologue: see there); its counted edits fill the first slots
        RecEnv env{st, b, go0, ax0, ay0, rec(V, R_SCORE), rec(V, R_BASE), rec(V, R_POSS),
                   rec_f64(V, R_MP)};
        // (cell 0 is the agent's: the agent planes' bits are there, and in no other cell)
        const u32 near = lane < 9 ? lds_plane_cell(buf, ps, V, near_cell_index(lane, ay0, ax0)) |
                                        (lane == 0 ? ps.agent16() : 0u)
                                  : 0u;
        OverlayT<NearCells> ov;
        ov.src = NearCells{ay0, ax0, near};
        ov.n = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ov.idx[k] = 0;
            ov.val[k] = 0;
        }
        if (lane == 0) act_reward = act_core(env, act, N, N, ka.ctp, ka.ctc, ov);
        act_reward = __builtin_amdgcn_readfirstlane(act_reward);
        echg = (1u << __builtin_amdgcn_readfirstlane(ov.n)) - 1u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            eidx[k] = __builtin_amdgcn_readfirstlane(ov.idx[k]);
            eval[k] = (u32)__builtin_amdgcn_readfirstlane((int)ov.val[k]);
        }
        go1 = __builtin_amdgcn_readfirstlane(env.go);
        ax1 = __builtin_amdgcn_readfirstlane(env.ax);
        ay1 = __builtin_amdgcn_readfirstlane(env.ay);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // no cell of the batch holds a bit outside the kept planes (board_zero), an
        // edited one included: said here, the planes not kept stay constants below
        if (K16) eval[k] &= K16;
        // the agent planes are rebuilt from the agent's new position below
        eval[k] &= ~ps.agent16();
    }
    // (SPLIT_EPI: the tail kernel reads the bonus table, at the distance handed over)
    const RecFields fl = SPLIT_EPI ? RecFields{V, go1, ax1, ay1, 0.0}
                                   : rec_fields(a, V, go1, ax1, ay1);
    const int hand_dist = SPLIT_EPI && a.bonus_period > 0 ? rec_bonus_dist(a, fl) : 0;

    u32 PB[32];
#pragma unroll
    for (int q = 0; q < 32; q++) PB[q] = ps.stored(q) ? buf[ps.pos(q) * 64 + lane] : 0u;
    wait_lgkm();
    constexpr u32 KEEP = K16 ? K16 : 0xFFFFu;
    // (W6: a caller-written start board is staged in two passes where it is read, below)
    if (roll < 0) {
        if (!W6) dma_board(st.start_board + off, buf, lane);
    } else pool_dma<KEEP, W6>(fx.pool, rec(V, R_LI), buf, lane);
    mux_edits4(PB, echg, eidx, eval, lane);
    // the agent planes: one word pair, the bit of the agent's cell after the action (the
    // rule changes no such cell: the host puts a plane in agent_planes only where the
    // agent's cell is frozen), read by the rule and the views, never loaded or stored
    {
        u32 aw[2];
        agent_words(fl.ay, fl.ax, lane, aw);
#pragma unroll
        for (int q = 0; q < 32; q++)
            if ((ps.agent16() >> (q & 15)) & 1u) PB[q] = aw[q >> 4];
    }
    // the derived planes (PlaneSlots): plane 15 is plane 2 with the action's edits in it;
    // plane 8 is the record's exit list (no action or rule moves, makes or removes an exit)
    if (ps.drv16() & 0x8000u) {
#pragma unroll
        for (int w = 0; w < 2; w++) PL(PB, 15, w) = PL(PB, 2, w);
    }
    if (ps.drv16() & 0x0100u) {
        u32 ew[2];
        exit_words(V, lane, ew);
#pragma unroll
        for (int w = 0; w < 2; w++) PL(PB, 8, w) = ew[w];
    }
    // held: changed cells that held a plane a change clears but never sets
    u32 cb[2], held[2];
    rule_planes(PB, cb, Geo64<SPAWN_PHILOX>{lane, ssrc, 0, 0}, sc, 0u, held);
    // (a lane mask, not two words held through the scores: such a lane stores those
    // planes for every changed word)
    const uint64_t held_lanes = __ballot((held[0] | held[1]) != 0u);
    // the new plane 3 is read by the stores alone: computed here, or the compiler sinks
    // it into them and keeps the rule's pair terms (eight registers) through the scores
#pragma unroll
    for (int w = 0; w < 2; w++) asm volatile("" : "+v"(PL(PB, 3, w)));
    __builtin_amdgcn_sched_barrier(0);

    // ---- scores over the new board and goals
    u32 PS[32];
    wait_vm();
    if (roll >= 0) {
        if (!W6) pool_planes_lds<KEEP>(buf, roll >> 16, roll & 0xFFFF, lane, PS);
    } else {
        if (W6) board_pairs_halves(st.start_board + off, buf, lane, PS);
        else read_pairs(buf, lane, PS);
        transpose32(PS);
        // planes no board holds: no start board either (as pool_planes_lds has them), so
        // neither path keeps a register for them
#pragma unroll
        for (int q = 0; q < 32; q++)
            if (!((KEEP >> (q & 15)) & 1u)) PS[q] = 0u;
    }
    int pts, scr, pos, side;
    const u32 gblack[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
    if (W6 && roll >= 0) {
        // one column word at a time: that word's start planes are read from LDS and
        // scored before the other's are read, so half of them are live at once (read
        // together, they are where this instance's register peak was)
        const int dy = roll >> 16, dx = roll & 0xFFFF;
        int p1, s1, o1, e1;
        pool_planes_lds_word<KEEP, 0>(buf, dy, dx, lane, PS);
        score_planes<false, 0, 1>(PB, GRAY ? gblack : gcol, PS, &pts, &scr, &pos, &side);
        __builtin_amdgcn_sched_barrier(0);
        pool_planes_lds_word<KEEP, 1>(buf, dy, dx, lane, PS);
        score_planes<false, 1, 2>(PB, GRAY ? gblack : gcol, PS, &p1, &s1, &o1, &e1);
        pts += p1;
        scr += s1;
        pos += o1;
        side += e1;
    } else
    score_planes(PB, GRAY ? gblack : gcol, PS, &pts, &scr, &pos, &side);
    const ScoreTotals tot = score_totals(pts, scr, pos, side);
    __builtin_amdgcn_sched_barrier(0);

    // ---- exits in the colour the epilogue gives them (update_exit_colors), then the
    // plane words that changed (all of them on a step into plane mode)
    const Words2 d9 = recolour_exits(
        PB, can_exit_now(fl.min_performance(), tot.score, fl.baseline(), tot.possible));
    u32 em[2] = {0u, 0u};           // the words the action's edits touched (this lane's)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((echg >> k) & 1u) {
            const int y = eidx[k] >> 6, x = eidx[k] & 63;
            const u32 bit = lane == 2 * (x >> 1) + (y >> 5) ? 1u << (y & 31) : 0u;
            em[x & 1] |= bit;
        }
    }
    u32 dw[2], dall[2];
#pragma unroll
    for (int w = 0; w < 2; w++) {
        dw[w] = cb[w] | em[w];                       // words whose cells changed
        dall[w] = em[w] | (((held_lanes >> lane) & 1ull) ? cb[w] : 0u);   // ... other planes
    }
    if (!pin || wave_or(dw[0] | dw[1] | d9.w[0] | d9.w[1])) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (!ps.stored(k)) continue;
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const u32 d = (k == 0 || k == 3 || k == 10 || k == 11) ? dw[w]
                              : k == 9 ? (dw[w] | d9.w[w]) : dall[w];
                if (!pin || d)
                    __builtin_nontemporal_store(PL(PB, k, w), &bp[ps.pos(k + 16 * w) * 64]);
            }
        }
    }
    const int ok = gok | SL_POK_BOARD_PLANES;
    if (ok != pok_all && lane == 0) st.planes_ok[b] = ok;
    if (OBS) {
        const bool rw = kernarg().fx.obs_rw != 0;
#pragma unroll
        for (int w = 0; w < 2; w++) {
            if (GRAY && rw) continue;                // (gray less white: nothing to add)
            u32 g0 = gcol[0][w], g1 = gcol[GRAY ? 0 : 1][w], g2 = gcol[GRAY ? 0 : 2][w];
            if (rw) {                                // white goals are background
                const u32 wh = g0 & g1 & g2;
                g0 &= ~wh;
                g1 &= ~wh;
                g2 &= ~wh;
            }
            const u32 b12 = PL(PB, 12, w), b13 = PL(PB, 13, w), b14 = PL(PB, 14, w);
            u32 c = b12 & g0;
            PL(PB, 12, w) = b12 ^ g0;
            const u32 x13 = b13 ^ g1;
            PL(PB, 13, w) = x13 ^ c;
            c = (b13 & g1) | (c & x13);
            const u32 x14 = b14 ^ g2;
            PL(PB, 14, w) = x14 ^ c;
            c = (b14 & g2) | (c & x14);
            PL(PB, 15, w) ^= c;                      // (the carry out of bit 15 drops)
        }
        transpose32(PB);
        lds_put_board(buf, lane, PB);               // (the start planes have been read)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (OBS >= 2) write_obs_channels<obs_esz(OBS)>(buf, vm, fl, b, lane);
        else write_obs(buf, fx, fl, b, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (SPLIT_EPI) {
        // the epilogue runs in k_env_epilogue_reset64, one lane per env: what it cannot
        // re-read from the state arrays goes out in the env's hand-over record, and with it
        // the bonus distance, which the wave has the whole ring for
        if (lane == 0)
            put_handover(handover_of(fx.scratch, st.B), b,
                         Handover{act_reward, tot.points, tot.score, tot.possible, tot.side,
                                  fl.go, fl.ax, fl.ay, hand_dist});
    } else {
    int reset = 0;
    if (lane == 0)
        reset = epilogue_core(st, a, b, fl, act_reward, tot.points, tot.score, tot.possible,
                              tot.side, ka.reward_out, ka.done_out, ka.flags_out, ka.ep_len_out,
                              ka.ep_rew_out);
    reset = __builtin_amdgcn_readfirstlane(reset);
    if (fx.fuse_reset && reset && lane == 0) queue_reset(fx.scratch, st.B, a.step, b);
    }
