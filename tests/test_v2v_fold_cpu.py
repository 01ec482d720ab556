"""CPU: which V2V plans end in the output fold (jh_v2v_fold -> v2v_fold_applies, csrc/conv3d_out_fold.hip).

The rule the plan builder asks, pinned over joints x grid x time batch: the fold takes at most 32 joints (64 input
channels, two column blocks of output channels) and a half-grid volume of whole 16-voxel row blocks, (G / 2)^3 a
multiple of 16, i.e. G a multiple of 8; everything else keeps the three launches.  Never a function of the time batch;
JH_V2V_FOLD=0 always gives the three launches and is read at every call.  Pure host arithmetic; no kernel runs here.
"""
import ctypes

import pytest

from jarvis_hybridnet_amd import _native as N
from tests.test_native_abi import header_symbols

JOINTS = (1, 5, 17, 23, 30, 40)
GRIDS = (16, 20, 24, 36, 64, 72)
BATCHES = (1, 9)


def folds(J, T, G):
    f = ctypes.c_int(-1)
    N.check(N.lib().jh_v2v_fold(J, T, G, ctypes.byref(f)))
    assert f.value in (0, 1)
    return bool(f.value)


def test_symbol_in_header_and_ctypes_table():
    assert "jh_v2v_fold" in header_symbols()
    assert "jh_v2v_fold" in N.symbols()
    assert hasattr(N.lib(), "jh_v2v_fold")


@pytest.mark.parametrize("J", JOINTS)
@pytest.mark.parametrize("G", GRIDS)
def test_decision_table(J, G, monkeypatch):
    monkeypatch.delenv("JH_V2V_FOLD", raising=False)
    want = J <= 32 and ((G // 2) ** 3) % 16 == 0
    got = [folds(J, T, G) for T in BATCHES]
    assert got[0] == got[1], "the decision must not depend on the time batch"
    assert got[0] == want
    monkeypatch.setenv("JH_V2V_FOLD", "0")
    assert [folds(J, T, G) for T in BATCHES] == [False, False]
    monkeypatch.setenv("JH_V2V_FOLD", "1")
    assert [folds(J, T, G) for T in BATCHES] == [want, want]


def test_flagship_and_shipped_shapes(monkeypatch):
    """The shapes the issue names: 23 joints at 64^3 (flagship) and 30 joints (cfg5) fold; the 72^3 grid folds
    (36^3 = 2916 row blocks); half grids of 10 and 18 voxels are ragged and do not."""
    monkeypatch.delenv("JH_V2V_FOLD", raising=False)
    assert folds(23, 32, 64) and folds(30, 32, 64) and folds(23, 16, 72)
    assert not folds(23, 3, 20) and not folds(23, 3, 36)


def test_knob_is_read_at_every_call(monkeypatch):
    monkeypatch.delenv("JH_V2V_FOLD", raising=False)
    assert folds(23, 1, 64)
    monkeypatch.setenv("JH_V2V_FOLD", "0")
    assert not folds(23, 1, 64)
    monkeypatch.delenv("JH_V2V_FOLD")
    assert folds(23, 1, 64)


def test_bad_arguments_are_refused():
    lib = N.lib()
    f = ctypes.c_int(0)
    assert lib.jh_v2v_fold(0, 1, 64, ctypes.byref(f)) != 0
    assert lib.jh_v2v_fold(23, 0, 64, ctypes.byref(f)) != 0
    assert lib.jh_v2v_fold(23, 1, 18, ctypes.byref(f)) != 0
    assert lib.jh_v2v_fold(23, 1, 64, None) != 0
