"""CPU: which kernel form a fused BiFPN node takes (jh_node_form -> choose_node, csrc/node_layer.hip).

The one function the network plan (EffTrackPlan::node) and the single-operator entry (jh_op_bifpn_node) both go
through, pinned row by row: node (channels, level, inputs, activation, images), time-batch class and whether the caller
could use the pooled output -> form, rows per segment, strips, segments, grid, block, dynamic LDS bytes and whether the
node writes the pooled output.  The expected values are those of the launchers this function replaced (their answers
were dumped before the change), not of the function under test.  Pure host arithmetic; no kernel runs here.
"""
import ast
import ctypes
import os
import subprocess
import sys

import pytest

from jarvis_hybridnet_amd import _native as N
from tests.test_native_abi import header_symbols

BY_SIZE, BELOW8, ATLEAST8 = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def form(case, cls=BY_SIZE, want_pool=0):
    """(name, seg_rows, strips, segs, grid.x, grid.y, block.x, lds, pool), or None where no form takes the node."""
    c, cout, h, w, modes, act, n = case
    m3 = (ctypes.c_int * 3)(*(list(modes) + [0] * (3 - len(modes))))
    name = ctypes.create_string_buffer(32)
    out = (ctypes.c_int32 * 8)()
    if N.lib().jh_node_form(c, cout, n, h, w, len(modes), m3, act, cls, want_pool, name, len(name), out):
        return None
    return (name.value.decode(),) + tuple(out)


def node_cases():
    """NODE_CASES of tests/test_hip_ops.py (read from the source: that module needs torch and a GPU)."""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_hip_ops.py")).read())
    for st in tree.body:
        if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", "") == "NODE_CASES":
            return ast.literal_eval(st.value)
    raise AssertionError("NODE_CASES not found")


# Every distinct node of a model's plan: (C, Cout, H, W, modes, act, images), class, want_pool -> the choice.
# (C, Cout, H, W, modes, act, n) as in NODE_CASES: modes 0 same level / 1 x2 up / 2 x4 up / 3 2x2 max-pool, act 2 SiLU.
MODEL_ROWS = [
    # small, 256-pixel crops, time batch 32 x 12 cameras
    ((56, 56, 8, 8, (0, 1), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 1, 384, 512, 48416, 0)),
    ((56, 56, 16, 16, (0, 1), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 2, 384, 512, 48416, 0)),
    ((56, 56, 32, 32, (0, 1), 2, 384), ATLEAST8, 0, ("rows_wave", 16, 2, 2, 4, 384, 64, 18208, 0)),
    ((56, 56, 64, 64, (0, 1), 2, 384), ATLEAST8, 1, ("rows_wave", 32, 4, 2, 8, 384, 64, 18208, 1)),
    ((56, 56, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wave", 16, 2, 2, 4, 384, 64, 18208, 0)),
    ((56, 56, 16, 16, (0, 0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 2, 384, 512, 48416, 0)),
    ((56, 56, 8, 8, (0, 0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 1, 384, 512, 48416, 0)),
    ((56, 56, 4, 4, (0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 1, 384, 512, 48416, 0)),
    ((56, 64, 64, 64, (0, 1, 2), 0, 384), ATLEAST8, 0, ("rows_wave", 16, 4, 4, 16, 384, 64, 18208, 0)),
    # small, 256-pixel crops, one 12-camera frame set
    ((56, 56, 8, 8, (0, 1), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 1, 12, 512, 48416, 0)),
    ((56, 56, 16, 16, (0, 1), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 2, 12, 512, 48416, 0)),
    ((56, 56, 32, 32, (0, 1), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 8, 12, 512, 48416, 0)),
    ((56, 56, 64, 64, (0, 1), 2, 12), BELOW8, 1, ("tile", 0, 0, 0, 32, 12, 512, 48416, 0)),
    ((56, 56, 32, 32, (0, 0, 3), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 8, 12, 512, 48416, 0)),
    ((56, 56, 16, 16, (0, 0, 3), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 2, 12, 512, 48416, 0)),
    ((56, 56, 8, 8, (0, 0, 3), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 1, 12, 512, 48416, 0)),
    ((56, 56, 4, 4, (0, 3), 2, 12), BELOW8, 0, ("tile", 0, 0, 0, 1, 12, 512, 48416, 0)),
    ((56, 64, 64, 64, (0, 1, 2), 0, 12), BELOW8, 0, ("tile", 0, 0, 0, 32, 12, 512, 48416, 0)),
    # medium, 256-pixel crops, time batch 32 x 12 cameras
    ((88, 88, 8, 8, (0, 1), 2, 384), ATLEAST8, 0, ("rows_wg", 8, 1, 1, 1, 384, 512, 41216, 0)),
    ((88, 88, 16, 16, (0, 1), 2, 384), ATLEAST8, 0, ("rows_pairs", 8, 1, 2, 192, 1, 512, 135936, 0)),
    ((88, 88, 32, 32, (0, 1), 2, 384), ATLEAST8, 0, ("rows_pairs", 32, 2, 1, 192, 1, 512, 135936, 0)),
    ((88, 88, 64, 64, (0, 1), 2, 384), ATLEAST8, 1, ("rows_pairs", 32, 4, 2, 768, 1, 512, 135936, 1)),
    ((88, 88, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_pairs", 32, 2, 1, 192, 1, 512, 135936, 0)),
    ((88, 88, 16, 16, (0, 0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 2, 384, 512, 78304, 0)),
    ((88, 88, 8, 8, (0, 0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 1, 384, 512, 78304, 0)),
    ((88, 88, 4, 4, (0, 3), 2, 384), ATLEAST8, 0, ("tile", 0, 0, 0, 1, 384, 512, 78304, 0)),
    ((88, 88, 64, 64, (0, 1, 2), 0, 384), ATLEAST8, 0, ("rows_pairs", 32, 4, 2, 768, 1, 512, 135936, 0)),
    # medium, 256-pixel crops, one 12-camera frame set
    ((88, 88, 8, 8, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 4, 4, 12, 512, 41216, 0)),
    ((88, 88, 16, 16, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 8, 8, 12, 512, 41216, 0)),
    ((88, 88, 32, 32, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 4, 2, 8, 16, 12, 512, 41216, 0)),
    ((88, 88, 64, 64, (0, 1), 2, 12), BELOW8, 1, ("rows_wg", 16, 4, 4, 16, 12, 512, 41216, 1)),
    ((88, 88, 32, 32, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 4, 2, 8, 16, 12, 512, 41216, 1)),
    ((88, 88, 16, 16, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 1, 8, 8, 12, 512, 41216, 1)),
    ((88, 88, 8, 8, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 1, 4, 4, 12, 512, 41216, 1)),
    ((88, 88, 4, 4, (0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 2, 2, 12, 512, 41216, 0)),
    ((88, 88, 16, 16, (0, 0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 8, 8, 12, 512, 41216, 0)),
    ((88, 88, 64, 64, (0, 1, 2), 0, 12), BELOW8, 0, ("rows_wg", 16, 4, 4, 16, 12, 512, 41216, 0)),
    # large, 256-pixel crops, time batch 32 x 12 cameras
    ((160, 160, 8, 8, (0, 1), 2, 384), ATLEAST8, 0, ("rows_wg", 8, 1, 1, 1, 384, 768, 71168, 0)),
    ((160, 160, 16, 16, (0, 1), 2, 384), ATLEAST8, 0, ("rows_wg", 8, 1, 2, 2, 384, 768, 71168, 0)),
    ((160, 160, 32, 32, (0, 1), 2, 384), ATLEAST8, 0, ("rows_wg", 32, 2, 1, 2, 384, 768, 71168, 0)),
    ((160, 160, 64, 64, (0, 1), 2, 384), ATLEAST8, 1, ("rows_wg", 64, 4, 1, 4, 384, 768, 71168, 1)),
    ((160, 160, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wg", 32, 2, 1, 2, 384, 768, 71168, 1)),
    ((160, 160, 16, 16, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wg", 8, 1, 2, 2, 384, 768, 71168, 1)),
    ((160, 160, 8, 8, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wg", 8, 1, 1, 1, 384, 768, 71168, 1)),
    ((160, 160, 4, 4, (0, 0), 2, 384), ATLEAST8, 0, ("rows_wg", 4, 1, 1, 1, 384, 768, 71168, 0)),
    ((160, 160, 16, 16, (0, 0, 0), 2, 384), ATLEAST8, 0, ("rows_wg", 8, 1, 2, 2, 384, 768, 71168, 0)),
    ((160, 160, 64, 64, (0, 1, 2), 0, 384), ATLEAST8, 0, ("rows_wg", 64, 4, 1, 4, 384, 768, 71168, 0)),
    # large, 256-pixel crops, one 12-camera frame set
    ((160, 160, 8, 8, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 4, 4, 12, 768, 71168, 0)),
    ((160, 160, 16, 16, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 8, 8, 12, 768, 71168, 0)),
    ((160, 160, 32, 32, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 4, 2, 8, 16, 12, 768, 71168, 0)),
    ((160, 160, 64, 64, (0, 1), 2, 12), BELOW8, 1, ("rows_wg", 16, 4, 4, 16, 12, 768, 71168, 1)),
    ((160, 160, 32, 32, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 4, 2, 8, 16, 12, 768, 71168, 1)),
    ((160, 160, 16, 16, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 1, 8, 8, 12, 768, 71168, 1)),
    ((160, 160, 8, 8, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 1, 4, 4, 12, 768, 71168, 1)),
    ((160, 160, 4, 4, (0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 2, 2, 12, 768, 71168, 0)),
    ((160, 160, 16, 16, (0, 0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 8, 8, 12, 768, 71168, 0)),
    ((160, 160, 64, 64, (0, 1, 2), 0, 12), BELOW8, 0, ("rows_wg", 16, 4, 4, 16, 12, 768, 71168, 0)),
    # medium, 320-pixel crops (levels 80 / 40 / 20 / 10 / 5), time batch 16 x 12 cameras
    ((88, 88, 10, 10, (0, 1), 2, 192), ATLEAST8, 0, ("rows_wg", 8, 1, 2, 2, 192, 512, 41216, 0)),
    ((88, 88, 20, 20, (0, 1), 2, 192), ATLEAST8, 0, ("rows_wg", 10, 2, 2, 4, 192, 512, 41216, 0)),
    ((88, 88, 40, 40, (0, 1), 2, 192), ATLEAST8, 0, ("rows_wg", 20, 3, 2, 6, 192, 512, 41216, 0)),
    ((88, 88, 80, 80, (0, 1), 2, 192), ATLEAST8, 1, ("rows_pairs", 40, 5, 2, 480, 1, 512, 135936, 1)),
    ((88, 88, 40, 40, (0, 0, 0), 2, 192), ATLEAST8, 1, ("rows_wg", 20, 3, 2, 6, 192, 512, 41216, 1)),
    ((88, 88, 20, 20, (0, 0, 0), 2, 192), ATLEAST8, 1, ("rows_wg", 10, 2, 2, 4, 192, 512, 41216, 1)),
    ((88, 88, 10, 10, (0, 0, 0), 2, 192), ATLEAST8, 1, ("rows_wg", 8, 1, 2, 2, 192, 512, 41216, 1)),
    ((88, 88, 5, 5, (0, 0), 2, 192), ATLEAST8, 0, ("rows_wg", 5, 1, 1, 1, 192, 512, 41216, 0)),
    ((88, 88, 20, 20, (0, 0, 0), 2, 192), ATLEAST8, 0, ("rows_wg", 10, 2, 2, 4, 192, 512, 41216, 0)),
    ((88, 88, 80, 80, (0, 1, 2), 0, 192), ATLEAST8, 0, ("rows_pairs", 40, 5, 2, 480, 1, 512, 135936, 0)),
    # medium, 320-pixel crops, one 12-camera frame set
    ((88, 88, 10, 10, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 5, 5, 12, 512, 41216, 0)),
    ((88, 88, 20, 20, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 2, 2, 10, 20, 12, 512, 41216, 0)),
    ((88, 88, 40, 40, (0, 1), 2, 12), BELOW8, 0, ("rows_wg", 4, 3, 10, 30, 12, 512, 41216, 0)),
    ((88, 88, 80, 80, (0, 1), 2, 12), BELOW8, 1, ("rows_wg", 16, 5, 5, 25, 12, 512, 41216, 1)),
    ((88, 88, 40, 40, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 4, 3, 10, 30, 12, 512, 41216, 1)),
    ((88, 88, 20, 20, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 2, 10, 20, 12, 512, 41216, 1)),
    ((88, 88, 10, 10, (0, 0, 0), 2, 12), BELOW8, 1, ("rows_wg", 2, 1, 5, 5, 12, 512, 41216, 1)),
    ((88, 88, 5, 5, (0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 3, 3, 12, 512, 41216, 0)),
    ((88, 88, 20, 20, (0, 0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 2, 10, 20, 12, 512, 41216, 0)),
    ((88, 88, 80, 80, (0, 1, 2), 0, 12), BELOW8, 0, ("rows_wg", 16, 5, 5, 25, 12, 512, 41216, 0)),
]

# What the stand-alone operator (class BY_SIZE, no pooled output) runs for NODE_CASES of tests/test_hip_ops.py, in order.
OP_ROWS = [
    ("tile", 0, 0, 0, 32, 3, 512, 48416, 0),
    ("tile", 0, 0, 0, 8, 3, 512, 48416, 0),
    ("tile", 0, 0, 0, 1, 3, 512, 48416, 0),
    ("tile", 0, 0, 0, 32, 3, 512, 48416, 0),
    ("tile", 0, 0, 0, 8, 3, 512, 78304, 0),
    ("rows_wave", 32, 4, 2, 8, 64, 64, 18208, 0),
    ("rows_wave", 16, 4, 4, 16, 64, 64, 18208, 0),
    ("rows_wave", 16, 2, 2, 4, 256, 64, 18208, 0),
    ("rows_wave", 24, 2, 2, 4, 192, 64, 18208, 0),
    ("rows_wave", 16, 2, 2, 4, 256, 64, 18208, 0),
    ("rows_pairs", 32, 4, 2, 128, 1, 512, 135936, 0),
    ("rows_pairs", 32, 4, 2, 128, 1, 512, 135936, 0),
    ("rows_pairs", 32, 2, 1, 128, 1, 512, 135936, 0),
    ("rows_pairs", 32, 2, 1, 128, 1, 512, 135936, 0),
    ("rows_pairs", 24, 2, 2, 192, 1, 512, 135936, 0),
    ("rows_pairs", 8, 1, 2, 1024, 1, 512, 135936, 0),
    ("tile", 0, 0, 0, 8, 3, 512, 139648, 0),
    ("rows_wg", 64, 4, 1, 4, 64, 768, 71168, 0),
    ("rows_wg", 64, 4, 1, 4, 64, 768, 71168, 0),
    ("rows_wg", 32, 2, 1, 2, 256, 768, 71168, 0),
    ("rows_wg", 32, 2, 1, 2, 256, 768, 71168, 0),
    ("rows_wg", 48, 2, 1, 2, 192, 768, 71168, 0),
    ("rows_wg", 8, 1, 2, 2, 2048, 768, 71168, 0),
    ("rows_wg", 8, 1, 1, 1, 2048, 768, 71168, 0),
    ("rows_wg", 8, 1, 1, 1, 2048, 768, 71168, 0),
    ("rows_wg", 4, 1, 1, 1, 4096, 768, 71168, 0),
    ("rows_wg", 2, 1, 1, 1, 4096, 768, 71168, 0),
    ("rows_wg", 12, 2, 2, 4, 512, 768, 71168, 0),
    ("rows_wg", 8, 3, 3, 9, 384, 768, 71168, 0),
    ("tile", 0, 0, 0, 1, 3, 512, 48416, 0),
    ("tile", 0, 0, 0, 15, 20, 512, 78304, 0),
    ("tile", 0, 0, 0, 6, 20, 512, 78304, 0),
    ("rows_wave", 40, 5, 2, 10, 43, 64, 28448, 0),
    ("rows_pairs", 40, 5, 2, 110, 1, 512, 135936, 0),
    ("tile", 0, 0, 0, 8, 255, 512, 78304, 0),
]

# The boundaries between the forms, at the smallest shapes that show them.
BOUNDARY_ROWS = [
    # 88 channels, 80 x 80: 430 items are one wave per strip, 440 = 110 workgroups of four pairs
    ((88, 88, 80, 80, (0, 1), 2, 43), BY_SIZE, 0, ("rows_wave", 40, 5, 2, 10, 43, 64, 28448, 0)),
    ((88, 88, 80, 80, (0, 1), 2, 44), BY_SIZE, 0, ("rows_pairs", 40, 5, 2, 110, 1, 512, 135936, 0)),
    # 88 channels, 32 x 32: 2040 against 2048 strips of eight rows
    ((88, 88, 32, 32, (0, 1), 2, 255), BY_SIZE, 0, ("tile", 0, 0, 0, 8, 255, 512, 78304, 0)),
    ((88, 88, 32, 32, (0, 1), 2, 256), BY_SIZE, 0, ("rows_pairs", 32, 2, 1, 128, 1, 512, 135936, 0)),
    # 88 channels on a ragged level: the workgroup form in a time-batch class only
    ((88, 88, 40, 40, (0, 1), 2, 192), ATLEAST8, 0, ("rows_wg", 20, 3, 2, 6, 192, 512, 41216, 0)),
    ((88, 88, 40, 40, (0, 1), 2, 192), BY_SIZE, 0, ("tile", 0, 0, 0, 15, 192, 512, 78304, 0)),
    ((88, 88, 40, 40, (0, 1), 2, 192), BELOW8, 0, ("rows_wg", 4, 3, 10, 30, 192, 512, 41216, 0)),
    # 56 channels below 32 pixels: the tile form in every class, whatever the launch size
    ((56, 56, 16, 16, (0, 1), 2, 4096), BY_SIZE, 0, ("tile", 0, 0, 0, 2, 4096, 512, 48416, 0)),
    ((56, 56, 16, 16, (0, 1), 2, 4096), BELOW8, 0, ("tile", 0, 0, 0, 2, 4096, 512, 48416, 0)),
    ((56, 56, 16, 16, (0, 1), 2, 4096), ATLEAST8, 0, ("tile", 0, 0, 0, 2, 4096, 512, 48416, 0)),
    # 56 channels, 32 x 32: 2040 against 2048 strips (class BY_SIZE only: a time-batch class does not look at the images)
    ((56, 56, 32, 32, (0, 1), 2, 255), BY_SIZE, 0, ("tile", 0, 0, 0, 8, 255, 512, 48416, 0)),
    ((56, 56, 32, 32, (0, 1), 2, 256), BY_SIZE, 0, ("rows_wave", 16, 2, 2, 4, 256, 64, 18208, 0)),
    ((56, 56, 32, 32, (0, 1), 2, 255), ATLEAST8, 0, ("rows_wave", 16, 2, 2, 4, 255, 64, 18208, 0)),
    ((56, 56, 32, 32, (0, 1), 2, 255), BELOW8, 0, ("tile", 0, 0, 0, 8, 255, 512, 48416, 0)),
    # 160 channels: every level down to 2 x 2 and widths that are no multiple of 16
    ((160, 160, 2, 2, (0, 0), 2, 12), ATLEAST8, 0, ("rows_wg", 2, 1, 1, 1, 12, 768, 71168, 0)),
    ((160, 160, 2, 2, (0, 0), 2, 12), BELOW8, 0, ("rows_wg", 2, 1, 1, 1, 12, 768, 71168, 0)),
    ((160, 160, 2, 2, (0, 0), 2, 12), BY_SIZE, 0, ("tile", 0, 0, 0, 1, 12, 512, 139648, 0)),
    ((160, 160, 24, 40, (0, 1, 2), 0, 12), ATLEAST8, 0, ("rows_wg", 8, 3, 3, 9, 12, 768, 71168, 0)),
    ((160, 160, 24, 40, (0, 1, 2), 0, 12), BELOW8, 0, ("rows_wg", 2, 3, 12, 36, 12, 768, 71168, 0)),
    ((160, 160, 24, 40, (0, 1, 2), 0, 12), BY_SIZE, 0, ("tile", 0, 0, 0, 9, 12, 512, 139648, 0)),
    # three same-level inputs, pooled output wanted: the workgroup form writes it, one wave per strip does not
    ((160, 160, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wg", 32, 2, 1, 2, 384, 768, 71168, 1)),
    ((56, 56, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 1, ("rows_wave", 16, 2, 2, 4, 384, 64, 18208, 0)),
    ((160, 160, 32, 32, (0, 0, 0), 2, 384), ATLEAST8, 0, ("rows_wg", 32, 2, 1, 2, 384, 768, 71168, 0)),
    # ... nor a node with more output than input channels, an odd height, or the tile form
    ((56, 64, 64, 64, (0, 1), 2, 384), ATLEAST8, 1, ("rows_wave", 32, 4, 2, 8, 384, 64, 18208, 0)),
    ((56, 56, 63, 64, (0, 1), 2, 384), ATLEAST8, 1, ("tile", 0, 0, 0, 32, 384, 512, 48416, 0)),
    # ReLU: the tile form only
    ((56, 56, 64, 64, (0, 1), 1, 12), BELOW8, 0, ("tile", 0, 0, 0, 32, 12, 512, 48416, 0)),
    # ... nor an odd width: the last pixel's lane would own pooled column W / 2, the first pixel of the next pooled row
    # (the same node one pixel wider writes it)
    ((160, 160, 6, 5, (0, 0, 0), 2, 12), ATLEAST8, 1, ("rows_wg", 6, 1, 1, 1, 12, 768, 71168, 0)),
    ((160, 160, 6, 6, (0, 0, 0), 2, 12), ATLEAST8, 1, ("rows_wg", 6, 1, 1, 1, 12, 768, 71168, 1)),
]

# Nodes that no form takes.
ERROR_ROWS = [
    ((56, 56, 64, 64, (0, 2, 1), 2, 384), ATLEAST8, 0),     # unsupported variant
    ((56, 56, 64, 64, (1, 1), 2, 384), ATLEAST8, 0),        # first input not at the node's own level
    ((56, 56, 64, 64, (0, 1), 1, 384), ATLEAST8, 0),        # ReLU on a row form
    ((160, 160, 32, 32, (0, 0, 0), 0, 384), ATLEAST8, 0),   # three same-level inputs without SiLU on a row form
    ((160, 160, 4, 4, (0, 0), 2, 384), ATLEAST8, 1),        # pooled output of the two-same-input variant
]


def test_symbol_in_header_and_ctypes_table():
    assert "jh_node_form" in header_symbols()
    assert "jh_node_form" in N.symbols()
    assert hasattr(N.lib(), "jh_node_form")


@pytest.mark.parametrize("case,cls,want_pool,want", MODEL_ROWS + BOUNDARY_ROWS)
def test_form_table(case, cls, want_pool, want):
    assert form(case, cls, want_pool) == want


def test_node_cases_of_the_op_test():
    cases = node_cases()
    assert len(cases) == len(OP_ROWS)
    for case, want in zip(cases, OP_ROWS):
        assert form(case) == want, case


def test_output_cases_run_what_the_plans_run():
    """tests/node_cases.py: every row of a time-batch class has a case with 3 (or 2) images, and jh_node_form gives that
    case the row's form, rows per segment, strips, segments, block, LDS and pooled output -- only the grid, which counts
    the images, may differ.  So tests/test_hip_node_outputs.py executes what the plans execute."""
    from tests import node_cases as NC
    cases = NC.cases()
    assert len({k.id for k in cases}) == len(cases)
    assert all(NC.runnable(r[0]) for r in MODEL_ROWS)
    assert [r[0][:4] for r in BOUNDARY_ROWS if not NC.runnable(r[0])] == [(56, 56, 63, 64)]   # (no such tensors)
    for node, cls, want_pool, want in MODEL_ROWS + [r for r in BOUNDARY_ROWS if r[1] != BY_SIZE and NC.runnable(r[0])]:
        k = NC.by_key(cases, node[:6], cls, want_pool)
        assert k.want[:4] + k.want[6:] == want[:4] + want[6:] and k.node[6] in (2, 3)   # (rows that differ in images only)
        got = form(k.node, cls, want_pool)
        assert got is not None, k.id
        assert got[:4] + got[6:] == want[:4] + want[6:], (k.id, got, want)
        # the largest tensor of the GPU file is 3 x 160 x 64 x 64 floats; 88 channels at 80 x 80 run with 2 images
        assert k.node[6] * max(k.node[0], k.node[1]) * k.node[2] * k.node[3] <= 3 * 160 * 64 * 64
    # every form, and every form that writes the pooled output, is among them
    assert {k.want[0] for k in cases} == set(NC.FORMS)
    assert {k.want[0] for k in cases if k.want[8]} == {"rows_wave", "rows_pairs", "rows_wg"}
    # the chains of the GPU file are made of table cases, and every node but the last writes its pooled output
    for c, cls, levels in NC.CHAINS:
        ks = NC.chain_nodes(cases, c, cls, levels)
        for k in ks:
            got = form(k.node, k.cls, k.want_pool)
            assert got[:4] + got[6:] == k.want[:4] + k.want[6:], (k.id, got)
        assert all(k.want[8] for k in ks[:-1]), (c, cls, levels)


@pytest.mark.parametrize("case,cls,want_pool", ERROR_ROWS)
def test_nodes_no_form_takes(case, cls, want_pool):
    assert form(case, cls, want_pool) is None
    assert N.lib().jh_last_error()


def test_bad_arguments_are_refused():
    name = ctypes.create_string_buffer(32)
    out = (ctypes.c_int32 * 8)()
    m3 = (ctypes.c_int * 3)(0, 1, 0)
    f = N.lib().jh_node_form
    assert f(56, 56, 3, 64, 64, 2, m3, 2, 0, 0, name, len(name), out) == 0
    assert f(56, 56, 3, 64, 64, 1, m3, 2, 0, 0, name, len(name), out) != 0
    assert f(56, 56, 3, 64, 64, 4, m3, 2, 0, 0, name, len(name), out) != 0
    assert f(56, 56, 3, 64, 64, 2, m3, 3, 0, 0, name, len(name), out) != 0
    assert f(56, 56, 3, 64, 64, 2, m3, 2, 3, 0, name, len(name), out) != 0
    assert f(56, 56, 0, 64, 64, 2, m3, 2, 0, 0, name, len(name), out) != 0
    assert f(56, 56, 3, 64, 64, 2, None, 2, 0, 0, name, len(name), out) != 0
    assert f(56, 56, 3, 64, 64, 2, m3, 2, 0, 0, None, 0, out) != 0
    assert f(56, 56, 3, 64, 64, 2, m3, 2, 0, 0, name, len(name), None) != 0


def test_node_operator_refuses_what_it_cannot_run():
    """jh_op_bifpn_node / jh_op_bifpn_node_ex check their arguments before they touch the GPU: a class outside 0 .. 2, a
    missing struct, and an up-sampled input of a node that is no whole multiple of its step (the 31-row x2 input of a
    63-row node has no source for output row 62)."""
    lib = N.lib()
    m3, w3 = (ctypes.c_int * 3)(0, 1, 0), (ctypes.c_float * 3)(0.5, 0.5, 0.0)
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value      # never read: the checks come first
    ex = N.OpNodeEx()
    ex.batch_class = 3
    args = (2, m3, w3, 2, 1, 56, 56, 64, 64, p, p, None, p, p, p, p)
    assert lib.jh_op_bifpn_node_ex(*args, ctypes.byref(ex), None) != 0
    assert b"batch_class" in lib.jh_last_error()
    assert lib.jh_op_bifpn_node_ex(*args, None, None) != 0
    ex.batch_class = ATLEAST8
    odd = (2, m3, w3, 2, 1, 56, 56, 63, 64, p, p, None, p, p, p, p)
    assert lib.jh_op_bifpn_node_ex(*odd, ctypes.byref(ex), None) != 0
    assert b"up-sampled" in lib.jh_last_error()
    assert lib.jh_op_bifpn_node(*odd, None) != 0
    assert b"up-sampled" in lib.jh_last_error()


def test_node_rows_knob_off_is_the_tile_form_everywhere():
    """JH_NODE_ROWS=0 (read once per process: a child process): every node of the tables takes the tile form."""
    rows = [r[:3] for r in MODEL_ROWS + BOUNDARY_ROWS + ERROR_ROWS[2:]] + [(c, BY_SIZE, 0) for c in node_cases()]
    # (the child loads the library alone: no package import, so the whole test stays well under a second)
    code = ("import ctypes\n"
            "f = ctypes.CDLL(%r).jh_node_form\n"
            "name, out = ctypes.create_string_buffer(32), (ctypes.c_int32 * 8)()\n"
            "for (c, cout, h, w, modes, act, n), cls, pool in %r:\n"
            "    m3 = (ctypes.c_int * 3)(*(list(modes) + [0] * (3 - len(modes))))\n"
            "    assert f(c, cout, n, h, w, len(modes), m3, act, cls, pool, name, len(name), out) == 0\n"
            "    assert name.value == b'tile' and out[7] == 0, (c, h, w, modes, cls)\n"
            "print('all tile')" % (N.lib()._name, rows))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, JH_NODE_ROWS="0"), cwd=ROOT,
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "all tile" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
