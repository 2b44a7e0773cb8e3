"""Episode log with side-effect scores: the batch counterpart of
``RecordingSafeLifeWrapper.log_episode`` (reference: safelife/env_wrappers.py:172-231).

The reference logs every finished episode of one env: its name, number, length, reward,
``performance_ratio()``, the initial green life, and -- ``record_side_effects`` -- the
side-effect score of the episode (side_effects.py:95-161).  Here ``sl_env_step`` resets a
finished env inside the step that finishes it, so the record is copied out first:
``EpisodeLog`` captures all B envs through ``sl_capture`` (final board, start board,
performance terms, ``num_steps``, spawn probability, ...; after the advance, before any
reset) into a ring of step slots.  Nothing is synchronised per step.  ``flush()`` (when
the ring fills, at ``close()``, or called by hand; records of a flush the full ring
forced are kept and returned by the next call) copies the ring to the host once, cuts
the finished episodes from the step flags, scores all of them in ONE device call
(``side_effect_scores``: the bit-sliced rollout where the board shape has one) and
writes one YAML record each; ``benchmarking.load_benchmarks`` reads the file back.
``scoring="device"`` copies only the flags and the scalar fields, gathers the finished
episodes' boards on the device and scores them there up to the EMD inputs
(``side_effect_scores(..., problems="device")``); only those boards come back.

This is meant for evaluation batches: a step with a capture attached leaves plane mode
(the board is kept as uint16 cells so it can be copied), and the ring holds
2 * ring * B boards.

Divergences, documented:
  * ``episode`` is the env's own episode number (1, 2, ...), as in ``TrajectoryRecorder``
    (the reference numbers episodes process-wide), and an extra ``env`` key carries the
    global env id;
  * the side-effect rollouts draw with Philox keyed by (cell, global env id, advance
    index, board), whatever RNG steps the env: episodes of one env share their draws at
    equal (cell, advance index).
"""
import ctypes
import os

import numpy as np

from . import _lib
from .cell_types import CellTypes, cell_name

HEADER = "# SafeLife benchmark data\n---\n"
_GREEN_LIFE = int(CellTypes.life | CellTypes.color_g)


def format_record(rec):
    """The YAML text of one episode record (the reference's layout, env_wrappers.py:
    195-220, plus the ``env`` key).  ``rec``: name, episode, env, length, reward,
    performance [completed, possible, cutoff], 'initial green', other ({key: number},
    optional), 'side effects' ({cell value: [emd, inaction mass]}, optional); other keys
    (EpisodeLog adds num_steps, spawn_prob and the boards) are not written."""
    completed, possible, cutoff = rec["performance"]
    msg = ("\n- name: {}\n  episode: {}\n  env: {}\n  length: {}\n  reward: {:0.3g}\n"
           "  performance: [{}, {}, {:0.3g}]\n  initial green: {}\n").format(
               rec["name"], rec["episode"], rec["env"], rec["length"], rec["reward"],
               completed, possible, cutoff, rec["initial green"])
    for key, val in (rec.get("other") or {}).items():
        msg += "  {}: {:0.4g}\n".format(key, val)
    if rec.get("side effects") is not None:
        msg += "  side effects:\n"
        msg += "\n".join("    {}: [{:0.2f}, {:0.2f}]".format(cell_name(cell), val[0], val[1])
                         for cell, val in rec["side effects"].items())
    return msg


def append_records(log_file, records):
    """Append the records' text to ``log_file`` (a path, or an object with write()); a
    new (absent or empty) file first gets the header."""
    text = "".join(format_record(r) for r in records)
    if hasattr(log_file, "write"):
        if hasattr(log_file, "tell") and log_file.tell() == 0:
            log_file.write(HEADER)
        log_file.write(text)
        if hasattr(log_file, "flush"):
            log_file.flush()
        return
    new = not os.path.exists(log_file) or os.path.getsize(log_file) == 0
    d = os.path.dirname(os.path.abspath(log_file))
    os.makedirs(d, exist_ok=True)
    with open(log_file, "a") as f:
        if new:
            f.write(HEADER)
        f.write(text)


class EpisodeLog:
    """Log every finished episode of a SafeLifeVecEnv (``auto_reset=True``).

    log_file: path or file object the records are appended to (None: only returned by
    ``flush``); record_side_effects / num_samples / side_effect_seed: the side-effect
    score of every episode (``side_effects.side_effect_scores`` with Philox draws);
    level_titles: names by pool level index (default ``level-<index>``);
    other_episode_data: {key: number or callable(global step count)} added to every
    record; ring: step slots captured between two flushes.
    scoring: 'host' copies the whole ring to the host at a flush and scores from there;
    'device' copies only the step flags and the scalar fields, gathers the finished
    episodes' boards on the device, scores them with
    ``side_effect_scores(..., problems="device")`` and copies just those boards back
    (the pinned host mirrors of the two board rings are not allocated).  Same records,
    same order; the side-effect EMDs are the same bits, the inaction sums may differ in
    the last bits (``side_effect_scores``).
    emd: 'host' solves the EMDs with ``sl_emd_cells_batch``; 'device' (with
    scoring='device' only) solves them where their cells are
    (``side_effect_scores(..., emd="device")``): the same bits.
    rollout_kw: further keywords of the rollout (``side_effect_densities``), such as
    ``kernel`` ('auto', 'generic', 'fast', 'bands', or 'mid' for boards of 33 to 64 rows)
    and ``max_keys``; rng, seed, env_ids and device are the log's own.
    """

    _FIELDS = (("score", "int32"), ("possible", "int32"), ("baseline", "int32"),
               ("num_steps", "int32"), ("spawn_prob", "float32"),
               ("min_performance", "float64"), ("episode_length", "int32"),
               ("episode_reward", "int32"), ("level_index", "int32"))

    def __init__(self, venv, log_file=None, record_side_effects=True, num_samples=1000,
                 side_effect_seed=0, level_titles=None, other_episode_data=None, ring=64,
                 scoring="host", emd="host", rollout_kw=None):
        if scoring not in ("host", "device"):
            raise ValueError("scoring must be 'host' or 'device', not %r" % (scoring,))
        if emd not in ("host", "device"):
            raise ValueError("emd must be 'host' or 'device', not %r" % (emd,))
        if emd == "device" and scoring != "device":
            raise ValueError("emd='device' needs scoring='device'")
        if not venv.auto_reset:
            raise ValueError("EpisodeLog needs auto_reset=True (episodes are cut at the "
                             "resets inside sl_env_step)")
        if getattr(venv, "_recorder", None) is not None:
            raise ValueError("a recorder is already attached to this env (one "
                             "TrajectoryRecorder or EpisodeLog at a time)")
        torch = venv.torch
        self.venv = venv
        self.log_file = log_file
        self.record_side_effects = bool(record_side_effects)
        self.num_samples = int(num_samples)
        self.side_effect_seed = int(side_effect_seed)
        self.level_titles = level_titles
        self.other_episode_data = dict(other_episode_data or {})
        B, R, H, W, dev = venv.B, int(ring), venv.H, venv.W, venv.device
        if R < 1:
            raise ValueError("ring must hold at least one step")
        self.R = R
        self.scoring = scoring
        self.emd = emd
        self.rollout_kw = dict(rollout_kw or {})
        taken = set(self.rollout_kw) & {"rng", "seed", "env_ids", "device", "problems", "emd"}
        if taken:
            raise ValueError("rollout_kw may not set %s" % ", ".join(sorted(taken)))
        self._ids = torch.arange(B, dtype=torch.int32, device=dev)
        self._board = torch.zeros((R, B, H, W), dtype=torch.uint16, device=dev)
        self._start = torch.zeros((R, B, H, W), dtype=torch.uint16, device=dev)
        self._flags = torch.zeros((R, B), dtype=torch.uint8, device=dev)
        self._t = {k: torch.zeros((R, B), dtype=getattr(torch, dt), device=dev)
                   for k, dt in self._FIELDS}
        # pinned host mirrors of the ring: a flush is async copies and one stream sync
        self._host = {k: torch.zeros(t.shape, dtype=t.dtype).pin_memory()
                      for k, t in self._ring().items()
                      if scoring == "host" or k not in ("board", "start")}
        self._cap = _lib.Capture()
        self._slot = 0
        self._pending = []           # records of the flushes the full ring forced
        self._ep = [int(x) for x in venv.st_t["episodes"].cpu().numpy()]
        self.records = 0
        venv._recorder = self

    def _ring(self):
        return dict(self._t, board=self._board, start=self._start, flags=self._flags)

    # --------------------------------------------------------------- per step
    def _next_capture(self):
        """The sl_capture of the coming step (called by SafeLifeVecEnv.step_async)."""
        if self._slot == self.R:
            self._drain()            # kept for the next flush() / close()
        s, c, B = self._slot, self._cap, self.venv.B
        hw = self.venv.H * self.venv.W
        c.n = B
        c.env = self._ids.data_ptr()
        c.board = self._board.data_ptr() + 2 * s * B * hw
        c.start_board = self._start.data_ptr() + 2 * s * B * hw
        c.flags = self._flags.data_ptr() + s * B
        for k, _ in self._FIELDS:
            t = self._t[k]
            setattr(c, k, t.data_ptr() + t.element_size() * s * B)
        self._slot += 1
        return ctypes.addressof(c)

    # ------------------------------------------------------------- episodes
    def _title(self, li):
        if self.level_titles is not None:
            return self.level_titles[li]
        return "level-%d" % li

    def flush(self):
        """Copy the captured slots to the host (async copies into pinned memory, one
        synchronisation), score the episodes that ended in them in one device call and
        append their records to the log file.  Returns the records (dicts) of every
        episode finished since the last flush() -- those of the flushes a full ring
        forced in between included."""
        self._drain()
        out, self._pending = self._pending, []
        return out

    def _drain(self):
        S = self._slot
        self._slot = 0
        if S == 0:
            return
        v = self.venv
        ring = self._ring()
        for k, m in self._host.items():
            m[:S].copy_(ring[k][:S], non_blocking=True)
        v.torch.cuda.current_stream(v.device).synchronize()
        fl = self._host["flags"][:S].numpy()
        ss, ii = np.nonzero(fl & 4)              # slot-major: the order the episodes ended
        if len(ss) == 0:
            return
        done = list(zip(ss.tolist(), ii.tolist()))
        h = {k: self._host[k][:S].numpy()[ss, ii] for k in self._t}
        if self.scoring == "device":
            # the finished episodes' boards, gathered on the device (indexed as int16: the
            # same bytes) and copied back alone
            si, ei = (v.torch.from_numpy(a).to(v.device) for a in (ss, ii))
            starts = self._start.view(v.torch.int16)[si, ei].view(v.torch.uint16)
            boards = self._board.view(v.torch.int16)[si, ei].view(v.torch.uint16)
            starts_h, boards_h = starts.cpu().numpy(), boards.cpu().numpy()
        else:
            starts = starts_h = self._host["start"][:S].numpy()[ss, ii]
            boards = boards_h = self._host["board"][:S].numpy()[ss, ii]
        gids = [v.env0 + int(i) for i in ii]
        scores = None
        if self.record_side_effects:
            from .side_effects import side_effect_scores
            scores = side_effect_scores(starts, boards, h["num_steps"], h["spawn_prob"],
                                        self.num_samples, rng="philox",
                                        seed=self.side_effect_seed, env_ids=gids,
                                        device=v.device, problems=self.scoring,
                                        emd=self.emd, **self.rollout_kw)
        step_count = v.global_counter.num_steps
        other = {k: float(val(step_count) if callable(val) else val)
                 for k, val in self.other_episode_data.items()}
        records = []
        for n, (s, i) in enumerate(done):
            base = int(h["baseline"][n])
            rec = {"name": self._title(int(h["level_index"][n])), "episode": self._ep[i],
                   "env": gids[n], "length": int(h["episode_length"][n]),
                   "reward": int(h["episode_reward"][n]),
                   "performance": [int(h["score"][n]) - base, int(h["possible"][n]) - base,
                                   max(0.0, float(h["min_performance"][n]))],
                   "initial green": int(np.sum((starts_h[n] | int(CellTypes.destructible))
                                               == _GREEN_LIFE)),
                   "num_steps": int(h["num_steps"][n]),
                   "spawn_prob": float(h["spawn_prob"][n]),
                   "start_board": starts_h[n], "final_board": boards_h[n],
                   "other": dict(other)}
            if scores is not None:
                rec["side effects"] = scores[n]
            self._ep[i] += 1
            records.append(rec)
        self.records += len(records)
        if self.log_file is not None:
            append_records(self.log_file, records)
        self._pending += records

    def on_reset(self, mask=None):
        """An explicit SafeLifeVecEnv.reset: episodes it cuts short are not logged."""
        self._drain()
        eps = self.venv.st_t["episodes"].cpu().numpy()
        m = None if mask is None else np.asarray(mask).reshape(-1)
        for i in range(self.venv.B):
            if m is None or m[i]:
                self._ep[i] = int(eps[i])

    def close(self):
        """Flush and detach from the env; returns what flush() returns."""
        out = self.flush()
        if getattr(self.venv, "_recorder", None) is self:
            self.venv._recorder = None
        return out
