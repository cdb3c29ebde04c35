"""The transposed-conv planner's decisions on a GPU-less host (csrc/convt_plan.hip) over a grid of
layer shapes, under the default tune state and with single keys changed, against
tests/golden/convt_plan.json (written by tests/golden/record_convt_plan.py):

  sizes  pis_convt2x2_wgrad_ws and pis_debug_convt2x2_wgrad_tile_splits, recorded from the library
         of the commit before the planner existed;
  algos  pis_debug_convt2x2_algo for the forward, the input gradient and the weight gradient, each
         with every pointer 16-byte aligned and with none, recorded from the planner once the bits
         of tests/test_convt_dispatch_gpu.py had matched that commit's on the MI355X. From then on
         it pins the policy.

The default state's tables are stored in full; every other state as the SHA-256 of its tables."""
import hashlib
import json
import os

import pytest

from physics_informed_image_segmentation_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convt_plan.json")

BATCHES = (1, 2, 8)
GRIDS = ((256, 256), (64, 64), (32, 32), (4, 64), (2, 32), (3, 16), (4, 4))
CINS = (8, 64, 128, 256, 512)
COUTS = (8, 32, 64, 128, 256)
# (key, value) set alone on top of the defaults; "default" is the empty state
STATES = ("default", "13=0", "13=1", "13=2", "13=3", "14=0", "14=1", "14=2", "31=0", "56=0")
SIZE_COLUMNS = ("B", "H", "W", "Cin", "Cout", "wgrad_ws", "tile_splits")
ALGO_COLUMNS = ("B", "H", "W", "Cin", "Cout", "fwd_aligned", "fwd_unaligned", "dgrad_aligned", "dgrad_unaligned",
                "wgrad_aligned", "wgrad_unaligned")


def in_wgrad_contract(Cin, Cout):
    """pis_convt2x2_wgrad's documented channel contract."""
    return Cin % 64 == 0 and Cout % 64 == 0


def shapes():
    return [(B, H, W, Cin, Cout) for B in BATCHES for H, W in GRIDS for Cin in CINS for Cout in COUTS]


def sizes(lib):
    """SIZE_COLUMNS rows; None outside the weight gradient's contract (the queries were undefined there)."""
    return [[*s, *((lib.pis_convt2x2_wgrad_ws(*s), lib.pis_debug_convt2x2_wgrad_tile_splits(*s))
                   if in_wgrad_contract(s[3], s[4]) else (None, None))] for s in shapes()]


def algos(lib):
    """ALGO_COLUMNS rows, contiguous operands (ld = channels)."""
    rows = []
    for s in shapes():
        B, H, W, Cin, Cout = s
        q = lib.pis_debug_convt2x2_algo
        rows.append([*s, q(0, *s, Cin, Cout, 1), q(0, *s, Cin, Cout, 0), q(1, *s, Cout, Cin, 1), q(1, *s, Cout, Cin, 0),
                     q(2, *s, Cin, Cout, 1), q(2, *s, Cin, Cout, 0)])
    return rows


def digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


class tuned:
    """Set the state's key for the block, restore it after."""

    def __init__(self, lib, state):
        self.lib = lib
        self.kv = None if state == "default" else tuple(int(v) for v in state.split("="))

    def __enter__(self):
        if self.kv:
            self.prev = self.lib.pis_tune(*self.kv)
            assert self.prev >= 0, self.lib.pis_last_error()

    def __exit__(self, *exc):
        if self.kv:
            self.lib.pis_tune(self.kv[0], self.prev)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_matches_the_fixture(golden):
    assert golden["size_columns"] == list(SIZE_COLUMNS) and golden["algo_columns"] == list(ALGO_COLUMNS)
    assert len(golden["sizes"]) == len(golden["algos"]) == len(shapes()) == 525
    assert sorted(golden["sizes_sha256"]) == sorted(golden["algos_sha256"]) == sorted(STATES)


def test_default_state_row_by_row(golden):
    lib = _hip.lib()
    for rows, want in ((sizes(lib), golden["sizes"]), (algos(lib), golden["algos"])):
        bad = [(g, w) for g, w in zip(rows, want) if g != w]
        assert not bad, f"{len(bad)} of {len(rows)} rows differ, first (got, want): {bad[0]}"


@pytest.mark.parametrize("state", STATES)
def test_single_key_states(golden, state):
    lib = _hip.lib()
    with tuned(lib, state):
        sz, al = sizes(lib), algos(lib)
    assert digest(sz) == golden["sizes_sha256"][state]
    assert digest(al) == golden["algos_sha256"][state]
    # a live check: the key moves decisions of this grid (31=0 moves none: the row-staged plain-operand
    # kernel it governs never takes the transposed conv's up-sampled dy)
    assert sum(a != b for a, b in zip(al, golden["algos"])) >= (0 if state in ("default", "31=0") else 100)


@pytest.mark.parametrize("state", ("13=0", "13=1", "13=2", "13=3", "56=0"))
def test_keys_13_and_56_do_not_move_the_workspace(golden, state):
    """The engine sizes the weight-gradient workspace once; keys 13 and 56 may change afterwards."""
    lib = _hip.lib()
    with tuned(lib, state):
        assert sizes(lib) == golden["sizes"]


def test_outside_the_contract():
    """The size queries answer 0 outside pis_convt2x2_wgrad's contract, as the 3x3 conv's do."""
    lib = _hip.lib()
    for s in ((1, 4, 4, 8, 64), (1, 32, 32, 96, 64), (1, 32, 32, 128, 32), (0, 32, 32, 128, 64)):
        assert lib.pis_convt2x2_wgrad_ws(*s) == 0 and lib.pis_debug_convt2x2_wgrad_tile_splits(*s) == 0
        assert lib.pis_debug_convt2x2_algo(2, *s, s[3], s[4], 1) == 0
