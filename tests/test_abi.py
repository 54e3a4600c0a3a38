"""The C-ABI boundary without a GPU: libpggan_hip.so loads, exports every function
include/pggan_hip.h declares, the ctypes table of pggan_amd/_lib.py declares each of them,
and the host-only entry points (step plan, workspace sizes, packed sizes) answer."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from pggan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pggan_hip.h")


def header_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpggan_hip.so not built")
    return _lib.load_library()


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = header_functions()
    assert len(names) >= 40, names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in include/pggan_hip.h but not exported: {missing}"
    unbound = [n for n in names if n not in _lib.SYMBOLS]
    assert not unbound, f"exported but missing from pggan_amd/_lib.py _SIGS: {unbound}"


def test_step_plan_on_the_host(lib):
    """pg_step_plan_* at the benchmark configuration (C5: stage 8, batch 4, bf16): one line
    per conv layer of G and D, the low-resolution kernel at 4^2 / 8^2, the persistent
    high-resolution tiles at 1024^2, a split workspace for the 16^2 convs."""
    depths = [512, 512, 512, 512, 256, 128, 64, 32, 16]
    ops = _lib.HipOps.__new__(_lib.HipOps)    # host-only: no tensors, no stream
    ops.lib, ops.dt = lib, _lib.PG_BF16
    ws, text = ops.step_plan(depths, 8, 4)
    lines = text.strip().splitlines()
    assert lines[0].startswith("stage 8 batch 4 dtype bf16")
    assert len(lines) == 1 + 2 * (1 + 2 * 8)
    assert ws > 0 and "splitK" in text
    assert any(l.startswith("G a") and "8x8" in l and "conv_lr" in l for l in lines), text
    assert any(l.startswith("D b") and "1024x1024" in l and "conv_hr" in l for l in lines), text
    # the weight gradient's kernel family: LDS-DMA at 1024^2, the register kernel at 4^2
    assert any(l.startswith("D b") and "1024x1024" in l and l.endswith(" dma") for l in lines), text
    assert any("   4x4 " in l and l.endswith(" reg") for l in lines), text
    with pytest.raises(RuntimeError):
        ops.step_plan(depths, 9, 4)          # stage beyond the depth list


def test_conv_support_query_agrees_with_the_launch(lib):
    """pg_conv3x3_supported and pg_conv3x3_fwd read one variant table: what the query calls
    supported the launch does not refuse as a bad argument, and what it calls unsupported the
    launch refuses.  Launch attempts with dummy pointers, so only where no device exists (a
    launch that passes the host checks ends in PG_ERR_HIP there).  Grid: the flag sets of the
    compile-time-flag rows, each also with one flag added or removed."""
    if torch.cuda.is_available():
        pytest.skip("makes launch attempts with dummy pointers: only without a device")
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    BF, ERR_ARG = _lib.PG_BF16, -1
    UPS, BIAS, LRELU, MASK, POOL, ACCUM, PN = (_lib.CONV_UPS_IN, _lib.CONV_BIAS, _lib.CONV_LRELU,
                                              _lib.CONV_MASK, _lib.CONV_POOL, _lib.CONV_ACCUM,
                                              _lib.CONV_PIXNORM)
    Y2B, AB, XB, PNB = _lib.CONV_Y2_BITS, _lib.CONV_AUX_BITS, _lib.CONV_X_BITS, _lib.CONV_PNBWD
    single = (UPS, BIAS, LRELU, MASK, POOL, ACCUM, PN, Y2B, AB, XB, PNB)
    rows = (0, BIAS | LRELU, MASK, PN | BIAS | LRELU, PNB, Y2B | BIAS | LRELU, AB | MASK,
            Y2B | POOL | BIAS | LRELU, AB | MASK | POOL, POOL, POOL | ACCUM, POOL | PNB,
            XB | MASK | UPS, XB | AB | MASK | UPS, PN | BIAS | LRELU | UPS)
    flag_sets = sorted({f for f in rows} | {f ^ s for f in rows for s in single})

    def cinp(c):
        return (c + 7) // 8 * 8 if c <= 16 else (c + 31) // 32 * 32

    def ask(B, H, cin, cout, fl):
        aux_cs = cout // 8 if fl & AB else cout
        y2_cs = max(2, cout // 8) if fl & Y2B else cout
        d = ctypes.byref(_lib.ConvDesc(B, H, H, cin, cout, cinp(cin), cout, aux_cs, y2_cs, fl, 0.2,
                                       1.0, cinp(cin) // 8))
        sup = lib.pg_conv3x3_supported(BF, d, 0)
        # y2 where the flags require it (the other rows run, or fall through, without it)
        rc = lib.pg_conv3x3_fwd(BF, d, p, p if fl & XB else None, p, p if fl & BIAS else None,
                                p if fl & (MASK | PNB) else None, p, p if fl & (Y2B | PNB) else None,
                                None, 0, None)
        return sup, rc

    n_sup = 0
    for B, H, cin, cout, fl in itertools.product((1, 4), (16, 256, 1024), (16, 32, 64), (16, 32, 64),
                                                 flag_sets):
        sup, rc = ask(B, H, cin, cout, fl)
        assert (rc != ERR_ARG) == bool(sup), (B, H, cin, cout, hex(fl), sup, rc, lib.pg_last_error())
        n_sup += sup
    assert n_sup > 1000
    # launches the query used to promise and the launcher refused
    assert ask(4, 256, 32, 16, XB | MASK) == (0, ERR_ARG)               # X_BITS without UPS_IN
    assert ask(4, 256, 32, 32, BIAS | LRELU | MASK | ACCUM | Y2B | AB) == (0, ERR_ARG)   # no such row
    assert ask(8, 1024, 128, 64, 0) == (0, ERR_ARG)                     # past the LDS-DMA input limit
    # the 512^2 tangent's own flags run (tile 14, without y2)
    assert ask(4, 256, 32, 64, MASK | POOL | AB)[0] == 1


# cin -> cout of test_gpu_ops.test_conv3x3_wgrad_gz_bits (B 2, H 16): one per GZ_BITS row
GZ_BITS_SHAPES = [(16, 32), (32, 64), (16, 16), (32, 16), (16, 24), (16, 64), (32, 48)]
WG_NROWS, WG_NROWS_BITS = 18, 7


def test_wgrad_support_query_agrees_with_the_launch(lib):
    """pg_conv3x3_wgrad_supported, pg_conv3x3_wgrad_workspace_size and pg_conv3x3_wgrad read one
    variant table (WG_ROWS): (a) the launch refuses as a bad argument exactly what the query
    calls unsupported; (b) the workspace the engine asks for without GZ_BITS holds the plan of
    the same launch with it.  Launch attempts with dummy pointers, so only without a device."""
    if torch.cuda.is_available():
        pytest.skip("makes launch attempts with dummy pointers: only without a device")
    from test_gpu_ops import WGRAD_CASES
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    BF, F32, ERR_ARG = _lib.PG_BF16, _lib.PG_F32, -1
    GZB, UPS = _lib.CONV_GZ_BITS, _lib.CONV_UPS_IN

    def cinp(c):
        return (c + 7) // 8 * 8 if c <= 16 else (c + 31) // 32 * 32

    def ask(B, H, cin, cout, fl, dtype=BF):
        mk = lambda f: ctypes.byref(_lib.ConvDesc(B, H, H, cin, cout, cinp(cin), (cout + 7) // 8 * 8,
                                                  0, 0, f, 0.2, 1.0, (cout + 7) // 8))
        sup = lib.pg_conv3x3_wgrad_supported(dtype, mk(fl))
        need = lib.pg_conv3x3_wgrad_workspace_size(dtype, mk(fl))
        plain = lib.pg_conv3x3_wgrad_workspace_size(dtype, mk(fl & ~GZB))
        ws = ctypes.cast((ctypes.c_float * 1)(), ctypes.c_void_p)     # never written: no device
        rc = lib.pg_conv3x3_wgrad(dtype, mk(fl), p, p, p if fl & GZB else None, 1.0, p, p, ws, need,
                                  None)
        return sup, rc, need, plain

    n_bits = 0
    for B, H, cin, cout, gzb, ups in itertools.product(
            (1, 4, 8), (4, 8, 16, 64, 512, 1024), (8, 16, 24, 32, 64, 128, 513),
            (8, 16, 24, 32, 48, 64, 128, 512), (0, GZB), (0, UPS)):
        if H >= 512 and max(cin, cout) > 64:
            continue
        sup, rc, need, plain = ask(B, H, cin, cout, gzb | ups)
        where = (B, H, cin, cout, hex(gzb | ups), sup, rc, lib.pg_last_error())
        assert (rc != ERR_ARG) == bool(sup), where                      # (a)
        assert 0 <= sup <= WG_NROWS, where
        if sup and gzb:
            assert plain >= need, where + (plain, need)                 # (b)
            n_bits += 1
    assert n_bits > 300
    # the tile without a GZ_BITS kernel: refused by both, taken without the flag
    for H in (16, 1024):
        assert ask(4, H, 32, 32, GZB)[:2] == (0, ERR_ARG)
        sup, rc = ask(4, H, 32, 32, 0)[:2]
        assert sup and rc != ERR_ARG
    # fp32: no GZ_BITS, everything else
    assert ask(4, 16, 32, 32, GZB, F32)[:2] == (0, ERR_ARG)
    sup, rc = ask(4, 16, 32, 32, UPS, F32)[:2]
    assert sup == 1 and rc != ERR_ARG
    # every row is reached by a GPU op test
    bits = [ask(2, 16, ci, co, GZB)[0] for ci, co in GZ_BITS_SHAPES]
    assert len(set(bits)) == WG_NROWS_BITS and all(bits), bits
    plain = {ask(B, H, ci, co, UPS if ups else 0)[0] for B, H, ci, co, ups in WGRAD_CASES}
    assert 0 not in plain
    assert len(plain) == WG_NROWS - WG_NROWS_BITS and not plain & set(bits), sorted(plain)


def test_merged_entry_points_reject_bad_arguments(lib):
    """The entry points that take their optional operand as a nullable argument refuse a flag
    without its operand, the fused-RGB flags without their own entry point, and bad shapes,
    on the host before any launch (the pointers here are never dereferenced), naming
    themselves in the message.  Shapes: 16x16, B 1, 16 -> 16 channels."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    BF = _lib.PG_BF16

    def desc(flags, H=16, aux_cs=0, xb_cs=0):
        return ctypes.byref(_lib.ConvDesc(1, H, 16, 16, 16, 16, 16, aux_cs, 0, flags, 0.2, 1.0, xb_cs))

    def fwd(d, xbits, aux=None, dtype=BF):
        return lib.pg_conv3x3_fwd(dtype, d, p, xbits, p, None, aux, p, None, None, 0, None)

    def from_rgb(src, mask_bits, ybits):
        return lib.pg_from_rgb(BF, 1, 16, 16, ctypes.byref(src), 0, p, None, 1.0, 0.2, None,
                               mask_bits, 16, p, ybits, None)

    img = _lib.ImgSrcDesc(p.value, None, None, None)
    mix = _lib.ImgSrcDesc(p.value, p.value, None, None)
    lin = _lib.LinearDesc(1, 16, 16, 0, 0, _lib.LIN_BIAS, 1.0, 0.2)
    rgbw = _lib.CONV_RGBW | _lib.CONV_MASK | _lib.CONV_AUX_BITS
    calls = {
        "conv3x3_fwd": [
            lambda: fwd(desc(_lib.CONV_X_BITS, xb_cs=2), None),        # flag without xbits
            lambda: fwd(desc(_lib.CONV_X_BITS, H=24, xb_cs=2), p),     # H not a power of two
            lambda: fwd(desc(rgbw, aux_cs=2), None, aux=p),            # RGBW: own entry point
            lambda: fwd(desc(0), None, dtype=7)],                      # no such dtype
        "conv3x3_wgrad": [
            lambda: lib.pg_conv3x3_wgrad(BF, desc(_lib.CONV_GZ_BITS, xb_cs=2), p, p, None, 1.0, p,
                                         None, None, 0, None)],
        "from_rgb": [lambda: from_rgb(img, p, p),                      # both bit operands
                     lambda: from_rgb(mix, None, None)],               # x1 without a / c
        "linear_fwd": [lambda: lib.pg_linear_fwd(BF, ctypes.byref(lin), p, p, None, None, p, None,
                                                 0, None)],
        "rgb_out_bwd_pn": [lambda: lib.pg_rgb_out_bwd_pn(BF, 1, 16, 16, 16, p, p, p, 1.0, p, 0.2, 16,
                                                         p, p, None, None, None)],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            assert fn() == -1, (name, i)
            assert name.encode() in lib.pg_last_error(), (name, i, lib.pg_last_error())
