"""The host half of the episode log: record text, file header, load_benchmarks, cell
names, and which kernel sl_side_effect_densities_k takes.  No GPU."""
import numpy as np

from safelife_amd import _lib
from safelife_amd.benchmarking import load_benchmarks
from safelife_amd.cell_types import CellTypes, cell_name, CELL_TYPE_NAMES, COLOR_NAMES
from safelife_amd.episode_log import HEADER, append_records, format_record

GREEN_LIFE = int(CellTypes.life | CellTypes.color_g)
RED_TREE = int(CellTypes.tree | CellTypes.color_r)

RECORD = {"name": "append-still-3", "episode": 7, "env": 12, "length": 153, "reward": -12,
          "performance": [5, 31, 0.01], "initial green": 14,
          "other": {"penalty_coef": 0.123456, "lr": 3e-4},
          "side effects": {GREEN_LIFE: [1.23456, 14.0], RED_TREE: [0.0, 2.499]}}

TEXT = """
- name: append-still-3
  episode: 7
  env: 12
  length: 153
  reward: -12
  performance: [5, 31, 0.01]
  initial green: 14
  penalty_coef: 0.1235
  lr: 0.0003
  side effects:
    life-green: [1.23, 14.00]
    tree-red: [0.00, 2.50]"""


def test_record_text_is_the_reference_layout():
    assert format_record(RECORD) == TEXT


def test_record_without_side_effects_ends_after_the_other_data():
    r = dict(RECORD)
    del r["side effects"]
    assert format_record(r) == TEXT[:TEXT.index("  side effects:")]


def test_header_once_then_appended(tmp_path):
    path = str(tmp_path / "sub" / "log.yaml")
    append_records(path, [RECORD])
    append_records(path, [RECORD, RECORD])
    text = open(path).read()
    assert text == HEADER + 3 * TEXT
    assert HEADER == "# SafeLife benchmark data\n---\n"


def test_load_benchmarks_round_trip(tmp_path):
    path = str(tmp_path / "log.yaml")
    plain = {"name": "b", "episode": 2, "env": 0, "length": 10, "reward": 2500.0,
             "performance": [0, 4, 0.0], "initial green": 0}
    third = dict(RECORD, name="c", episode=3, length=9,
                 **{"side effects": {GREEN_LIFE: [0.5, 1.0]}})
    append_records(path, [RECORD, plain])
    append_records(path, [third])
    d = load_benchmarks(path)
    assert d["name"].tolist() == ["append-still-3", "b", "c"]
    assert d["episode"].tolist() == [7, 2, 3]
    assert d["env"].tolist() == [12, 0, 12]
    assert d["length"].tolist() == [153, 10, 9]
    assert d["reward"].tolist() == [-12, 2500.0, -12]          # %0.3g: 2.5e+03
    assert d["performance"].tolist() == [[5, 31, 0.01], [0, 4, 0.0], [5, 31, 0.01]]
    assert d["initial green"].tolist() == [14, 0, 14]
    assert d["penalty_coef"].tolist() == [0.1235, 0, 0.1235]   # absent: 0
    assert sorted(d["side effects"]) == ["life-green", "tree-red"]
    assert d["side effects"]["life-green"].tolist() == [[1.23, 14.0], [0.0, 0.0], [0.5, 1.0]]
    assert d["side effects"]["tree-red"].tolist() == [[0.0, 2.5], [0.0, 0.0], [0.0, 0.0]]
    assert isinstance(d["length"], np.ndarray)


def test_cell_names_over_types_and_colours():
    want_types = ["empty", "life", "hard-life", "wall", "crate", "plant", "tree", "ice-cube",
                  "parasite", "weed", "spawner", "hard-spawner", "exit", "fountain"]
    assert [n for _, n in CELL_TYPE_NAMES] == want_types
    values = {"empty": 0, "life": 9, "hard-life": 1, "wall": 16, "crate": 0x8014,
              "plant": 0x8015, "tree": 17, "ice-cube": 0x8074, "parasite": 0x55, "weed": 0x35,
              "spawner": 0x98, "hard-spawner": 0x90, "exit": 0x110, "fountain": 0x30}
    colours = ["gray", "red", "green", "yellow", "blue", "magenta", "cyan", "white"]
    assert list(COLOR_NAMES) == colours
    for tname, v in values.items():
        for c, cname in enumerate(colours):
            assert cell_name(v | (c << 9)) == tname + "-" + cname
            assert cell_name(np.uint16(v | (c << 9))) == tname + "-" + cname
    assert cell_name(2) == "unknown-gray"                      # an agent is no cell type
    assert cell_name(0x1009 | (2 << 9)) == "unknown-green"


def test_side_effect_kernel_choice():
    L = _lib.lib()
    P, S = _lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM
    for shape in ((64, 64), (25, 25), (2, 2), (32, 64)):
        assert L.sl_side_effect_kernel(*shape, P) == _lib.SL_KERNEL_FAST, shape
    for shape in ((128, 128), (33, 20), (20, 65)):
        assert L.sl_side_effect_kernel(*shape, P) == _lib.SL_KERNEL_GENERIC, shape
    for shape in ((64, 64), (25, 25)):
        assert L.sl_side_effect_kernel(*shape, S) == _lib.SL_KERNEL_GENERIC, shape
    assert hasattr(L, "sl_side_effect_densities_k")
