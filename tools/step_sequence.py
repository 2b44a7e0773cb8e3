"""Two steps of one small env per step kernel family and rng mode (tests/step_cases.py),
plus 64x64 with packed views and 64x64 with a capture: run under a kernel trace, the
ordered kernel names are the launch sequence of sl_env_step.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/step_sequence.py
    python tools/step_sequence.py --names OUT > profiles/step_sequence.txt

--names prints the traced kernel names in start order, one per line, keeping the library's
own kernels (k_*; torch's fills and copies between the steps are left out)."""
import csv
import glob
import os
import re
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("safelife-k2_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))


def names(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if re.search(r"\bk_[a-z0-9_]+", name):
            print(name)


def run():
    import torch
    import step_cases
    from safelife_amd.recorder import TrajectoryRecorder

    def two_steps(env):
        for t in range(2):
            g = torch.Generator(device="cuda:0").manual_seed(t)
            env.step_async(torch.randint(0, 9, (step_cases.B,), dtype=torch.int32,
                                         device="cuda:0", generator=g))
        torch.cuda.synchronize()

    for name, H, W, family, rng in step_cases.CASES:
        two_steps(step_cases.make_env(H, W, rng))
    two_steps(step_cases.c3_env())
    two_steps(step_cases.c3_env(compute_obs=True, view_shape=(33, 33)))
    env = step_cases.c3_env()
    # (two steps fill two slots of the recorder's ring: nothing is written to disk)
    TrajectoryRecorder(env, os.path.join(tempfile.gettempdir(), "{env}-{episode_num}"), [0, 5])
    two_steps(env)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--names":
        names(sys.argv[2])
    else:
        run()
