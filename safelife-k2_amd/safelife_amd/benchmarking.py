"""Reading episode logs (reference: safelife/benchmarking.py ``load_benchmarks``).

``EpisodeLog`` (episode_log.py) writes one YAML record per finished episode, in the
layout of the reference's ``RecordingSafeLifeWrapper.log_episode``; ``load_benchmarks``
turns such a file into arrays, one entry per episode.  PyYAML is imported when the
function is called.
"""
import numpy as np

SIDE = "side effects"


def load_benchmarks(logfile):
    """{field: array [n_episodes, ...]} of a log file, plus ``'side effects'``:
    {cell name: array [n_episodes, 2]}.  An episode without a field counts 0 there, one
    without a side-effect entry [0.0, 0.0]."""
    import yaml
    with open(logfile) as f:
        episodes = yaml.safe_load(f) or []
    fields = sorted({k for ep in episodes for k in ep if k != SIDE})
    cells = sorted({k for ep in episodes for k in (ep.get(SIDE) or {})})
    out = {k: np.array([ep.get(k, 0) for ep in episodes]) for k in fields}
    out[SIDE] = {c: np.array([(ep.get(SIDE) or {}).get(c, [0.0, 0.0]) for ep in episodes])
                 for c in cells}
    return out
