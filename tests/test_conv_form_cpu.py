"""CPU: which kernel form a convolution layer takes (jh_conv_form -> choose_conv, csrc/conv_layer.hip).

The one function the network plans (Plan::add_conv) and the single-operator entries (jh_op_conv, jh_op_conv_operand)
both go through, pinned row by row: layer, use (bias / fused statistics / gate), precision level and the three knobs
JH_WINO, JH_WINO_PW, JH_DECONV4_WINDOW.  The knobs are set with monkeypatch between calls of one process, which also
shows that they are read when a layer is made, not once per process.  Pure host arithmetic; no kernel runs here.
"""
import ctypes

import pytest

from jarvis_hybridnet_amd import _native as N
from tests.test_native_abi import header_symbols

KNOBS = ("JH_WINO", "JH_WINO_PW", "JH_DECONV4_WINDOW")
NONE, TENSOR, RECIPE = 0, 1, 2


def form(layer, bias=False, stats=False, gate=NONE, prec=0, in_px=0):
    nd, kind, k, stride, pad, cin, cout = layer
    name = ctypes.create_string_buffer(32)
    N.check(N.lib().jh_conv_form(nd, kind, k, stride, pad, cin, cout, int(bias), int(stats), gate, prec, in_px,
                                 name, len(name)))
    return name.value.decode()


def conv(nd, k, stride, pad, cin, cout):
    return (nd, 0, k, stride, pad, cin, cout)


def deconv2d(cin, cout):
    return (2, 1, 4, 2, 1, cin, cout)


V2V_RES, V2V_FRONT, V2V_POOL = conv(3, 3, 1, 1, 46, 46), conv(3, 3, 2, 1, 23, 46), conv(3, 2, 2, 0, 46, 92)

# layer, use, precision, environment, form
ROWS = [
    (V2V_RES, dict(bias=True, stats=True), 0, {}, "wino"),
    (V2V_RES, dict(bias=True, stats=True), 0, {"JH_WINO": "0"}, "mfma"),
    (V2V_RES, dict(bias=True, stats=True), 1, {}, "wino_bf16x3"),
    (V2V_FRONT, dict(bias=True, stats=True), 0, {}, "mfma_tappair"),
    (V2V_FRONT, dict(bias=True, stats=True), 1, {}, "conv_bf16x3"),
    (V2V_POOL, dict(bias=True, stats=True), 0, {}, "mfma"),
    (V2V_POOL, dict(bias=True, stats=True), 1, {}, "mfma"),
    (V2V_POOL, dict(bias=True, stats=True), 2, {}, "mfma"),
    (deconv2d(64, 23), {}, 0, {}, "mfma_window"),
    (deconv2d(64, 23), {}, 0, {"JH_DECONV4_WINDOW": "0"}, "mfma_paired"),
    (deconv2d(64, 23), {}, 1, {}, "deconv4_bf16x3"),
    (deconv2d(64, 23), dict(stats=True), 0, {}, "mfma_paired"),
    (deconv2d(64, 23), dict(stats=True), 1, {}, "mfma_paired"),
    (deconv2d(64, 30), {}, 0, {}, "mfma_paired"),
    (deconv2d(64, 30), {}, 0, {"JH_DECONV4_WINDOW": "2"}, "mfma_window"),
    (deconv2d(64, 40), {}, 0, {}, "mfma"),
    (deconv2d(88, 23), {}, 0, {}, "mfma_window"),
    (deconv2d(88, 23), dict(stats=True), 0, {}, "mfma"),
    (deconv2d(64, 1), {}, 0, {}, "deconv_c1"),
    (deconv2d(64, 1), {}, 1, {}, "deconv_c1"),
    (deconv2d(64, 1), {}, 2, {}, "deconv_c1"),
    (conv(2, 3, 1, 1, 8, 16), dict(stats=True), 1, {}, "mfma"),
    (conv(2, 3, 1, 1, 8, 16), dict(stats=True), 2, {}, "conv_bf16x3"),
    (conv(2, 3, 2, 1, 3, 16), dict(stats=True, in_px=4), 2, {}, "mfma"),
    (conv(2, 1, 1, 0, 96, 16), dict(stats=True, gate=TENSOR), 0, {}, "mfma"),
    (conv(2, 1, 1, 0, 96, 16), dict(stats=True, gate=TENSOR), 2, {}, "mfma"),
    (conv(2, 1, 1, 0, 96, 16), dict(stats=True, gate=RECIPE), 0, {}, "mfma"),
    (conv(2, 1, 1, 0, 96, 16), dict(stats=True, gate=RECIPE), 2, {}, "mfma"),
]


def test_symbol_in_header_and_ctypes_table():
    assert "jh_conv_form" in header_symbols()
    assert "jh_conv_form" in N.symbols()
    assert hasattr(N.lib(), "jh_conv_form")
    assert N.lib().jh_abi_version() == 4


@pytest.mark.parametrize("layer,use,prec,env,want", ROWS)
def test_form_table(layer, use, prec, env, want, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert form(layer, prec=prec, **use) == want


def test_knobs_are_read_at_every_call(monkeypatch):
    """One process, the knob flipped between calls: each call sees the value of its moment."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    use = dict(bias=True, stats=True)
    assert form(V2V_RES, **use) == "wino"
    monkeypatch.setenv("JH_WINO", "0")
    assert form(V2V_RES, **use) == "mfma"
    monkeypatch.setenv("JH_WINO", "1")
    assert form(V2V_RES, **use) == "wino"
    assert form(deconv2d(64, 23)) == "mfma_window"
    monkeypatch.setenv("JH_DECONV4_WINDOW", "0")
    assert form(deconv2d(64, 23)) == "mfma_paired"
    monkeypatch.delenv("JH_DECONV4_WINDOW")
    assert form(deconv2d(64, 23)) == "mfma_window"


def test_the_one_channel_head_needs_the_bare_use():
    """deconv_c1 takes the ConvTranspose2d k4 s2 p1 with one output channel only without bias, statistics and gate."""
    assert form(deconv2d(64, 1)) == "deconv_c1"
    assert form(deconv2d(64, 1), bias=True) != "deconv_c1"
    assert form(deconv2d(64, 1), stats=True) != "deconv_c1"
    assert form(deconv2d(64, 1), gate=TENSOR) != "deconv_c1"
    assert form(deconv2d(64, 2)) != "deconv_c1"


def test_bad_arguments_are_refused():
    name = ctypes.create_string_buffer(32)
    lib = N.lib()
    assert lib.jh_conv_form(4, 0, 3, 1, 1, 8, 8, 0, 0, 0, 0, 0, name, len(name)) != 0
    assert lib.jh_conv_form(2, 0, 3, 1, 1, 8, 8, 0, 0, 3, 0, 0, name, len(name)) != 0
    assert lib.jh_conv_form(2, 0, 3, 1, 1, 8, 8, 0, 0, 0, 3, 0, name, len(name)) != 0
    assert lib.jh_conv_form(2, 0, 3, 1, 1, 8, 8, 0, 0, 0, 0, 0, None, 0) != 0
