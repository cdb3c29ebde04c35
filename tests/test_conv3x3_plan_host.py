"""The 3x3-conv planner's decisions on a GPU-less host (csrc/conv3x3_plan.hip): the six size and
format queries of include/pis_capi.h over a grid of layer shapes, under the default tune state and
with single keys changed, against the table recorded before the planner existed
(tests/golden/conv3x3_plan.json, written by tests/golden/record_conv3x3_plan.py).

The default state's table is stored in full; every other state as the SHA-256 of its table."""
import hashlib
import json
import os

import pytest
import torch

from physics_informed_image_segmentation_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_plan.json")

BATCHES = (1, 2, 8)
GRIDS = ((512, 512), (256, 256), (128, 128), (64, 64), (32, 32), (48, 80), (30, 34), (8, 32), (6, 10), (4, 4), (2, 2))
CINS = (1, 4, 32, 64, 128, 256, 512, 1024)
COUTS = (36, 64, 128, 256, 512, 1024)
# (key, value) set alone on top of the defaults; "default" is the empty state
STATES = ("default", "7=1", "8=0", "8=2", "9=2048", "10=3", "10=0", "11=0", "15=0", "22=0", "26=0", "27=0", "29=0",
          "29=2", "29=4", "47=1", "49=4")
HUGE = 1 << 40
COLUMNS = ("B", "H", "W", "Cin", "Cout", "ex_ws", "keep_bytes", "fmt_fwd", "fmt_dgrad", "filter_bytes_fwd",
           "filter_bytes_dgrad", "dgrad_direct_huge_ws", "dgrad_direct_zero_ws", "wgrad_ws")


def in_wgrad_contract(Cin, Cout):
    """pis_conv3x3_wgrad's documented channel contract."""
    return Cout % 64 == 0 and (Cin == 1 or Cin % 64 == 0)


def table(lib):
    """One row per shape of the grid, COLUMNS order; wgrad_ws is None outside its contract."""
    rows = []
    for B in BATCHES:
        for H, W in GRIDS:
            for Cin in CINS:
                for Cout in COUTS:
                    s = (B, H, W, Cin, Cout)
                    rows.append([*s, lib.pis_conv3x3_ex_ws(*s), lib.pis_conv3x3_keep_bytes(*s),
                                 lib.pis_conv3x3_filter_format(*s, 0), lib.pis_conv3x3_filter_format(*s, 1),
                                 lib.pis_conv3x3_filter_bytes(*s, 0), lib.pis_conv3x3_filter_bytes(*s, 1),
                                 lib.pis_conv3x3_dgrad_direct(*s, Cout, HUGE), lib.pis_conv3x3_dgrad_direct(*s, Cout, 0),
                                 lib.pis_conv3x3_wgrad_ws(*s) if in_wgrad_contract(Cin, Cout) else None])
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
    assert golden["columns"] == list(COLUMNS)
    assert len(golden["default"]) == len(BATCHES) * len(GRIDS) * len(CINS) * len(COUTS) == 1584
    assert sorted(golden["sha256"]) == sorted(STATES)


def test_default_state_row_by_row(golden):
    rows = table(_hip.lib())
    bad = [(got, want) for got, want in zip(rows, golden["default"]) if got != want]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first (got, want): {bad[0]}"
    assert digest(rows) == golden["sha256"]["default"]


@pytest.mark.parametrize("state", STATES[1:])
def test_single_key_states(golden, state):
    lib = _hip.lib()
    before = lib.pis_tune(int(state.split("=")[0]), -1)
    with tuned(lib, state):
        rows = table(lib)
    assert lib.pis_tune(int(state.split("=")[0]), -1) == before
    assert digest(rows) == golden["sha256"][state]
    # a live check: the key moves rows of this grid (10=3 moves none: the policy only asks
    # whether key 10 is >= 3, and the default is 4)
    assert sum(a != b for a, b in zip(rows, golden["default"])) >= (0 if state == "10=3" else 24)


@pytest.mark.parametrize("shape", [(1, 32, 32, 64, 36), (1, 32, 32, 64, 100), (1, 32, 32, 4, 64), (1, 32, 32, 32, 64),
                                   (8, 512, 512, 3, 64), (1, 30, 34, 64, 36), (1, 4, 4, 96, 96), (2, 6, 10, 1, 36)])
def test_wgrad_ws_outside_the_contract_is_zero(shape):
    """Shapes pis_conv3x3_wgrad rejects: the size query answers 0 (it used to divide by a zero
    tile count) and the process is alive to say so; the compute call still reports the contract."""
    lib = _hip.lib()
    assert not in_wgrad_contract(shape[3], shape[4])
    assert lib.pis_conv3x3_wgrad_ws(*shape) == 0
    if torch.cuda.is_available():
        return  # a compute call that slipped through validation would launch with the stand-in pointers below
    B, H, W, Cin, Cout = shape
    rc = lib.pis_conv3x3_wgrad(1, Cin if Cin > 1 else 1, 1, Cout, 1, 1, B, H, W, Cin, Cout, 0, 1, HUGE, 0)
    assert rc == -1 and b"Cout must be a multiple of 64" in lib.pis_last_error()
