#!/usr/bin/env python3
"""A/B of the side-effect rollout kernels: side_effects.side_effect_densities with
kernel="generic" (one per-cell launch per advance) against the bit-sliced rollout (four
launches per call): kernel="fast" (one wave per board), on 128x128 boards kernel="bands"
(four waves per board), on boards of 33 to 64 rows kernel="mid" (one wave per board), or on
other boards past 64 rows or columns kernel="wide" (a wave per band of 32 rows).

    python tools/side_effect_bench.py [--out profiles/side_effect_rollout_ab.json]
    python tools/side_effect_bench.py --boards 128 [--out profiles/side_effect_rollout128_ab.json]
    python tools/side_effect_bench.py --boards mid [--out profiles/side_effect_rollout_mid_ab.json]
    python tools/side_effect_bench.py --boards wide [--out profiles/side_effect_rollout_wide_ab.json]

Default: the C3 pool's 64x64 boards and the C2 pool's 25x25 boards (tests/golden/pools),
E in {1, 64, 1024} episodes, generic against fast.  --boards 128: the C5 pool's 128x128
boards, E in {1, 64, 256} (at 256 the maps are already 1 GiB), generic against bands.
--boards mid: boards of 33x32 (the narrowest SL_KERNEL_AUTO would take), 48x48, 64x48 and
-- for the record only -- 33x20, E in {1, 64, 1024}, generic against mid; no pool of these
shapes is committed, so the boards are those of tools/mid_bench.py's seeded generator
(make_levels).  The record also says what kAutoTakesMidRollout (sl_board.hip) follows from
it: true if at every shape of W >= 32 and every E the slowest mid run beats the fastest
generic run.
--boards wide: boards of 96x96, 100x100, 65x128 and 40x128 (the shapes of tools/wide_bench.py,
from the same generator), E in {1, 64, 256}, generic against wide.  The kernel is opt-in
whatever the numbers say; the record lists the cases it does not win.
num_steps = 1000, num_samples = 1000, max_keys = 16 (at 64 the 64x64
maps of 1024 episodes are 4 GiB).  Three runs of each kernel, interleaved (generic, fast,
generic, ...); every timed call runs in a child process of its own under a time limit,
after a small warm-up call of the same kernel, with torch.cuda.synchronize around it.
The time is that of the whole Python call: rollouts, the copy of the maps to the host
and the per-key dicts, the same work for both kernels.  A child that fails or runs out
of time ends the tool: nothing more is started on the GPU.

    python tools/side_effect_bench.py --problems host [--boards 64|128] [--measure ...]
    python tools/side_effect_bench.py --problems device ...    (the same A/B, device first)

--problems: the A/B of where the EMDs' cells are selected instead, by the same protocol
(three runs of each form, interleaved, beginning with the named one; a child process per
timed call): side_effect_scores(problems="host") against problems="device", kernel
"auto", on the C3 pool's 64x64 boards (E in {1, 64, 1024}) or the C5 pool's 128x128
boards (E in {1, 64, 256}); the record is profiles/side_effect_problems_ab.json, one
"boards" entry per run of the tool.  Two things are timed, each in children of its own:
  inputs   the rollout until every EMD's inputs (selected cells, inaction sum) are on the
           host: side_effect_densities plus earth_mover_distance's numpy selection per
           key, against side_effect_problems;
  scores   the whole side_effect_scores call.
The final board is the start board without six neighbouring living cells (the local
change an agent makes).  On the 64x64 still-life boards the EMD problems are then tens of
cells.  On the 128x128 navigation boards the spawners make the two runs differ in
thousands of cells whatever the agent did, and the exact host EMD of one such problem
takes from seconds to minutes in either form, so "scores" is timed there only when asked
for by --measure scores, and --episodes E keeps it to one episode count (E = 1: one
problem of 7 427 cells, half a minute of host EMD in either form).  A "scores" child also
reports episode 0's EMDs, and the tool ends if the two forms ever disagree on them.

    python tools/side_effect_bench.py --emd host|device [--episodes E] [--pool c3_64x64]

--emd: the A/B of where the EMDs are solved, by the same protocol (three runs of each form,
interleaved, beginning with the named one; a child process per timed call after a small
warm-up call of the same form; torch.cuda.synchronize around the call): the whole
side_effect_scores(problems="device", emd="host") call against emd="device", kernel
"auto", on the C3 pool's 64x64 boards and the C2 pool's 25x25 boards, E in {1, 64, 1024},
the same local change as final board; the record is profiles/side_effect_emd_ab.json.
After its timed call a child solves the same problems once more, untimed, and reports
what the pivot cap and the size limit of sl_emd_cells_device rest on: the problems with
cells, the share of them left to the host by size and by the cap, the largest pivots /
(n + m) and the largest cell count.  Every child also reports a digest of all EMDs, and
the tool ends if the two forms ever disagree on it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "safelife-k2_amd"))

POOLS = {"c3_64x64": "c3_prune_still_64.npz", "c2_25x25": "c2_append_still_25.npz",
         "c5_128x128": "c5_navigation_128.npz"}
# generated boards (tools/mid_bench.py: make_levels), by shape
MID_SHAPES = {"mid_33x32": (33, 32), "mid_48x48": (48, 48), "mid_64x48": (64, 48),
              "mid_33x20": (33, 20)}
WIDE_SHAPES = {"wide_96x96": (96, 96), "wide_100x100": (100, 100), "wide_65x128": (65, 128),
               "wide_40x128": (40, 128)}
GENERATED = dict(MID_SHAPES, **WIDE_SHAPES)
AUTO_MID_MIN_W = 32         # kAutoMidMinW (sl_board.hip)
STEPS = SAMPLES = 1000
MAX_KEYS = 16
# --boards: the pools, the episode counts, the kernel set against generic, the record
SETS = {"64": (("c3_64x64", "c2_25x25"), (1, 64, 1024), "fast", "side_effect_rollout_ab.json"),
        "128": (("c5_128x128",), (1, 64, 256), "bands", "side_effect_rollout128_ab.json"),
        "mid": (tuple(MID_SHAPES), (1, 64, 1024), "mid", "side_effect_rollout_mid_ab.json"),
        "wide": (tuple(WIDE_SHAPES), (1, 64, 256), "wide", "side_effect_rollout_wide_ab.json")}
RUNS = 3
CALL_LIMIT_S = 240
# --problems: pool, episode counts, what is timed by default
PROBLEM_SETS = {"64": ("c3_64x64", (1, 64, 1024), ("inputs", "scores")),
                "128": ("c5_128x128", (1, 64, 256), ("inputs",))}
PROBLEMS_RECORD = "side_effect_problems_ab.json"
# --emd: the pools, the episode counts, the record
EMD_SET = (("c3_64x64", "c2_25x25"), (1, 64, 1024))
EMD_RECORD = "side_effect_emd_ab.json"


def _pool_boards(pool):
    import numpy as np
    if pool in GENERATED:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from mid_bench import make_levels
        return np.stack([d["board"] for d in make_levels(*GENERATED[pool])])
    return np.load(os.path.join(REPO, "tests", "golden", "pools", POOLS[pool]))["board"]


def one_call(pool, E, kernel):
    import numpy as np
    import torch
    from safelife_amd.side_effects import side_effect_densities
    board = _pool_boards(pool)
    init = np.ascontiguousarray(board[np.arange(E) % len(board)])
    final = np.roll(init, 1, axis=2)
    dev = torch.device("cuda:0")
    init_d, final_d = torch.from_numpy(init).to(dev), torch.from_numpy(final).to(dev)
    kw = dict(rng="philox", seed=1, max_keys=MAX_KEYS, kernel=kernel, device=dev)
    side_effect_densities(init_d[:1], final_d[:1], [2], 0.3, 2, **kw)        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = side_effect_densities(init_d, final_d, [STEPS] * E, 0.3, SAMPLES, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"seconds": dt, "keys_episode0": len(out[0][0])}))


def _local_change(board):
    """The board without the six living cells nearest to its first one."""
    import numpy as np
    b = board.copy()
    yy, xx = np.nonzero((b & 1) != 0)
    near = np.argsort(np.abs(yy - yy[0]) + np.abs(xx - xx[0]), kind="stable")[:6]
    b[yy[near], xx[near]] = 0
    return b


def _host_inputs(init_d, final_d, steps, sp, samples, **kw):
    """What problems="host" does before its EMDs: the dense maps to the host, then
    earth_mover_distance's selection per key."""
    import numpy as np
    from safelife_amd.side_effects import side_effect_densities
    zeros = np.zeros(tuple(init_d.shape[-2:]))
    out = []
    for ina, act in side_effect_densities(init_d, final_d, steps, sp, samples, **kw):
        d = {}
        for key in set(ina) | set(act):
            a, b = ina.get(key, zeros), act.get(key, zeros)
            gap = np.abs(a - b)
            sel = gap > 1e-3 * np.max(gap)
            ys, xs = np.nonzero(sel)
            d[key] = (a[sel], b[sel], ys, xs, np.sum(a))
        out.append(d)
    return out


def one_problems_call(pool, E, form, measure):
    import numpy as np
    import torch
    from safelife_amd.side_effects import side_effect_problems, side_effect_scores
    board = np.load(os.path.join(REPO, "tests", "golden", "pools", POOLS[pool]))["board"]
    levels = np.stack([board[k] for k in range(len(board))])
    finals = np.stack([_local_change(b) for b in levels])
    pick = np.arange(E) % len(levels)
    dev = torch.device("cuda:0")
    init_d = torch.from_numpy(np.ascontiguousarray(levels[pick])).to(dev)
    final_d = torch.from_numpy(np.ascontiguousarray(finals[pick])).to(dev)
    kw = dict(rng="philox", seed=1, max_keys=MAX_KEYS, kernel="auto", device=dev)
    if measure == "scores":
        def call(a, b, steps, samples):
            return side_effect_scores(a, b, steps, 0.3, samples, problems=form, **kw)
    elif form == "host":
        def call(a, b, steps, samples):
            return _host_inputs(a, b, steps, 0.3, samples, **kw)
    else:
        def call(a, b, steps, samples):
            return side_effect_problems(a, b, steps, 0.3, samples, **kw)
    call(init_d[:1], final_d[:1], [2], 2)                                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call(init_d, final_d, [STEPS] * E, SAMPLES)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cells = (sum(len(v[0]) for d in out for v in d.values()) if measure == "inputs" else None)
    emds = (sorted((int(k), float(v[0]).hex()) for k, v in out[0].items())
            if measure == "scores" else None)
    print(json.dumps({"seconds": dt, "keys_episode0": len(out[0]), "selected_cells": cells,
                      "emd_episode0": emds}))


def problems_main(args):
    pool, es, measures = PROBLEM_SETS[args.boards]
    if args.measure:
        measures = (args.measure,)
    if args.episodes:
        es = (args.episodes,)
    forms = (args.problems, "device" if args.problems == "host" else "host")
    out_path = args.out or os.path.join(REPO, "profiles", PROBLEMS_RECORD)
    from safelife_amd import _lib
    result = {"num_steps": STEPS, "num_samples": SAMPLES, "max_keys": MAX_KEYS, "runs": RUNS,
              "build_id": _lib.build_id(), "kernel": "auto", "pool": pool,
              "final_board": "start board without six neighbouring living cells",
              "timed": {"inputs": "rollout until every EMD's inputs are on the host, seconds",
                        "scores": "whole side_effect_scores call, seconds"},
              "cases": []}
    for E in es:
        for measure in measures:
            case = {"E": E, "measure": measure, "host": [], "device": []}
            for _ in range(RUNS):
                for form in forms:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-problems",
                                        pool, str(E), form, measure], stdout=subprocess.PIPE,
                                       text=True, timeout=CALL_LIMIT_S)
                    if p.returncode != 0:
                        print("child failed (%s E=%d %s %s): rc %d"
                              % (pool, E, form, measure, p.returncode))
                        return 1
                    got = json.loads(p.stdout.strip().splitlines()[-1])
                    case[form].append(got["seconds"])
                    if got["selected_cells"] is not None:
                        case["selected_cells_%s" % form] = got["selected_cells"]
                    if got["emd_episode0"] is not None:
                        if case.setdefault("emd_episode0", got["emd_episode0"]) \
                                != got["emd_episode0"]:
                            print("the forms disagree on episode 0's EMDs (E=%d)" % E)
                            return 1
            case["device_wins"] = max(case["device"]) < min(case["host"])
            case["ratio_best_host_over_worst_device"] = min(case["host"]) / max(case["device"])
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    record = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            record = json.load(f)
    if args.boards in record and (args.measure or args.episodes):
        # a partial run adds its cases to the record of the full one
        old = record[args.boards]
        done = {(c["E"], c["measure"]) for c in result["cases"]}
        result["cases"] = sorted([c for c in old["cases"] if (c["E"], c["measure"]) not in done]
                                 + result["cases"], key=lambda c: (c["E"], c["measure"]))
        if old["build_id"] != result["build_id"]:
            result["build_id"] = {"E=%d %s" % (c["E"], c["measure"]):
                                  (result["build_id"] if (c["E"], c["measure"]) in done
                                   else old["build_id"]) for c in result["cases"]}
    record[args.boards] = result
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


def _local_boards(pool, E, dev):
    """E start boards of the pool (its levels in turn) and the same boards after the local
    change, on the device."""
    import numpy as np
    import torch
    board = np.load(os.path.join(REPO, "tests", "golden", "pools", POOLS[pool]))["board"]
    levels = np.stack([board[k] for k in range(len(board))])
    finals = np.stack([_local_change(b) for b in levels])
    pick = np.arange(E) % len(levels)
    return (torch.from_numpy(np.ascontiguousarray(levels[pick])).to(dev),
            torch.from_numpy(np.ascontiguousarray(finals[pick])).to(dev))


def one_emd_call(pool, E, form):
    import hashlib
    import numpy as np
    import torch
    from safelife_amd import _lib
    from safelife_amd.side_effects import (_problems_host, emd_problem_nodes,
                                           side_effect_scores)
    dev = torch.device("cuda:0")
    init_d, final_d = _local_boards(pool, E, dev)
    kw = dict(rng="philox", seed=1, max_keys=MAX_KEYS, kernel="auto", device=dev)
    side_effect_scores(init_d[:1], final_d[:1], [2], 0.3, 2, problems="device", emd=form, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = side_effect_scores(init_d, final_d, [STEPS] * E, 0.3, SAMPLES, problems="device",
                             emd=form, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    digest = hashlib.sha256(repr([sorted((int(k), float(v[0]).hex()) for k, v in d.items())
                                  for d in out]).encode()).hexdigest()[:16]
    # untimed: the same problems once more, for the kernel's status of every read slot
    pr = _problems_host(init_d, final_d, [STEPS] * E, 0.3, SAMPLES, emd="device", **kw)
    pr.cells_to_host()
    read = (np.arange(MAX_KEYS)[None, :] < pr.n_keys[:, None]).reshape(-1)
    sizes = np.diff(pr.offsets)
    has = read & (sizes > 0)
    st = pr.emd_status
    nodes = emd_problem_nodes(pr.p, pr.q, pr.offsets)
    solved = has & (st > 0) & (nodes > 0)
    ratio = float((st[solved] / nodes[solved]).max()) if solved.any() else 0.0
    n = max(1, int(has.sum()))
    print(json.dumps({"seconds": dt, "digest": digest, "problems": int(has.sum()),
                      "cells": int(sizes[has].sum()), "largest_cells": int(sizes.max()),
                      "share_by_size": float((has & (st == _lib.SL_EMD_ST_TOOBIG)).sum()) / n,
                      "share_by_cap": float((has & (st == _lib.SL_EMD_ST_PIVOTS)).sum()) / n,
                      "largest_pivots_per_node": ratio}))


def emd_main(args):
    pools, es = EMD_SET
    if args.pool:
        pools = (args.pool,)
    if args.episodes:
        es = (args.episodes,)
    forms = (args.emd, "device" if args.emd == "host" else "host")
    out_path = args.out or os.path.join(REPO, "profiles", EMD_RECORD)
    from safelife_amd import _lib
    result = {"num_steps": STEPS, "num_samples": SAMPLES, "max_keys": MAX_KEYS, "runs": RUNS,
              "build_id": _lib.build_id(), "kernel": "auto", "problems": "device",
              "final_board": "start board without six neighbouring living cells",
              "timed": "whole side_effect_scores call, seconds", "cases": []}
    stats = ("problems", "cells", "largest_cells", "share_by_size", "share_by_cap",
             "largest_pivots_per_node")
    for pool in pools:
        for E in es:
            case = {"pool": pool, "E": E, "host": [], "device": []}
            for _ in range(RUNS):
                for form in forms:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-emd",
                                        pool, str(E), form], stdout=subprocess.PIPE, text=True,
                                       timeout=CALL_LIMIT_S)
                    if p.returncode != 0:
                        print("child failed (%s E=%d %s): rc %d" % (pool, E, form, p.returncode))
                        return 1
                    got = json.loads(p.stdout.strip().splitlines()[-1])
                    case[form].append(got["seconds"])
                    if case.setdefault("digest", got["digest"]) != got["digest"]:
                        print("the forms disagree on the EMDs (%s E=%d)" % (pool, E))
                        return 1
                    for k in stats:
                        case[k] = got[k]
            case["device_wins"] = max(case["device"]) < min(case["host"])
            case["ratio_best_host_over_worst_device"] = min(case["host"]) / max(case["device"])
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    if os.path.exists(out_path) and (args.pool or args.episodes):
        # a partial run adds its cases to the record of the full one
        with open(out_path) as f:
            old = json.load(f)
        done = {(c["pool"], c["E"]) for c in result["cases"]}
        if old["build_id"] != result["build_id"]:
            result["build_id"] = {"%s E=%d" % (c["pool"], c["E"]): old["build_id"]
                                  if isinstance(old["build_id"], str)
                                  else old["build_id"]["%s E=%d" % (c["pool"], c["E"])]
                                  for c in old["cases"] if (c["pool"], c["E"]) not in done}
            result["build_id"].update({"%s E=%d" % k: _lib.build_id() for k in done})
        result["cases"] = sorted([c for c in old["cases"] if (c["pool"], c["E"]) not in done]
                                 + result["cases"], key=lambda c: (c["pool"], c["E"]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", choices=sorted(SETS), default="64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--problems", choices=("host", "device"), default=None)
    ap.add_argument("--measure", choices=("inputs", "scores"), default=None)
    ap.add_argument("--episodes", type=int, default=None,
                    help="with --problems or --emd: one E only")
    ap.add_argument("--emd", choices=("host", "device"), default=None)
    ap.add_argument("--pool", choices=sorted(POOLS), default=None, help="with --emd: one pool only")
    ap.add_argument("--one-emd", nargs=3, metavar=("POOL", "E", "FORM"))
    ap.add_argument("--one", nargs=3, metavar=("POOL", "E", "KERNEL"))
    ap.add_argument("--one-problems", nargs=4, metavar=("POOL", "E", "FORM", "MEASURE"))
    args = ap.parse_args()
    if args.one:
        one_call(args.one[0], int(args.one[1]), args.one[2])
        return 0
    if args.one_problems:
        pool, E, form, measure = args.one_problems
        one_problems_call(pool, int(E), form, measure)
        return 0
    if args.one_emd:
        pool, E, form = args.one_emd
        one_emd_call(pool, int(E), form)
        return 0
    if args.emd:
        return emd_main(args)
    if args.problems:
        return problems_main(args)
    pools, es, new, record = SETS[args.boards]
    out_path = args.out or os.path.join(REPO, "profiles", record)
    from safelife_amd import _lib
    result = {"num_steps": STEPS, "num_samples": SAMPLES, "max_keys": MAX_KEYS, "runs": RUNS,
              "build_id": _lib.build_id(), "timed": "whole side_effect_densities call, seconds",
              "cases": []}
    for pool in pools:
        for E in es:
            case = {"pool": pool, "E": E, "generic": [], new: []}
            for _ in range(RUNS):
                for kernel in ("generic", new):
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", pool,
                                        str(E), kernel], stdout=subprocess.PIPE, text=True,
                                       timeout=CALL_LIMIT_S)
                    if p.returncode != 0:
                        print("child failed (%s E=%d %s): rc %d" % (pool, E, kernel, p.returncode))
                        return 1
                    case[kernel].append(json.loads(p.stdout.strip().splitlines()[-1])["seconds"])
            case["%s_wins" % new] = max(case[new]) < min(case["generic"])
            case["speedup_worst_%s_vs_best_generic" % new] = min(case["generic"]) / max(case[new])
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    if args.boards == "mid":
        lost = ["%s E=%d" % (c["pool"], c["E"]) for c in result["cases"]
                if MID_SHAPES[c["pool"]][1] >= AUTO_MID_MIN_W and not c["mid_wins"]]
        result["boards"] = "tools/mid_bench.py make_levels(H, W), 32 levels, seed 0"
        result["auto_min_w"] = AUTO_MID_MIN_W
        result["auto_takes_mid"] = not lost
        result["auto_cases_lost"] = lost
    if args.boards == "wide":
        result["boards"] = "tools/mid_bench.py make_levels(H, W), 32 levels, seed 0"
        result["opt_in"] = True
        result["cases_not_won"] = ["%s E=%d" % (c["pool"], c["E"]) for c in result["cases"]
                                   if not c["wide_wins"]]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
