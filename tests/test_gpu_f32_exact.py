"""The fp32 parity kernels of csrc/f32path.hip - the 13 ep24_f32_* entry points - against tests/f32_reference.py, through the C ABI.
tests/test_f32_reference.py shows without a GPU that the references equal torch in float64 (conv2d, batch_norm, max_pool2d,
interpolate, unfold and their autograd) and that every mutant of its list is rejected on these inputs.

Every buffer sits between two guards of 64 sentinel elements and whole buffers are compared: the pad columns of strided rows, the gaps
between weight rows, the head's rows of other levels and every buffer a call must not write.  NaN equals NaN; every other pattern only
itself.  A case is either bit for bit (integer or dyadic operands make every intermediate exact, or leave one sequence of separately
rounded IEEE operations: the library is built without FMA contraction) or under the bound that f32_reference derives for it from the
kernel's expression (a double sum rounded once, half an ulp more per further fp32 operation, expf within 2 ulp); the roundings are
counted in f32_reference's docstring.  No tolerance comes from a kernel's output.

Bit for bit: conv, transposed conv, weight gradient, pool backward and column sums on integer draws; BatchNorm forward (save, running
statistics, y) and backward (sums as float64 patterns, dz, gamma_grad, beta_grad) on the exact draws with M = 1, 2, 256 and act 0, 2, 3;
the pool forward in values and index planes (ties, -inf windows, one and two NaN); both upsample directions and rows_copy on every
draw; the stem pack on random patterns; the decode gradient on dyadic draws.  Under a bound: the same on normal draws, every SiLU
case and every M that is no power of two.

engine.unit passes the block's input as the residual and a fresh activation or a concat slot as the output, never residual = y, so
the aliased form is not a case.  The second trip of the grid-stride loops needs more than 1 048 576 x 256 elements, about a gibibyte
per buffer, and is left out.

Largest err / bound measured on an MI355X (the tests print them as F32-ERR before they assert; 586 cases, 2 s):
  conv forward 0.99773, transposed 0.99838 (both k 7, s 2 on the 6 x 4 map), stem form 0.99982, weight gradient 0.99613: a sum that falls
      close to the middle of two fp32 numbers; the share of the double additions went unused
  BatchNorm forward 0.99607 on the integer draws at M = 255 and 0.9999987 at M = 257, C = 1, both in save: S / 255 and S / 257 of a short
      sum S have the periods 00000001 and 0000000011111111, which end next to a tie; y alone 0.86 at most (SiLU included)
  BatchNorm backward 0.88182 (act 3, M = 1), 0.80000 (act 0 and 2, M = 1), SiLU 0.30473, integer draws with M no power of two 0.41825
  pool backward 1.00000: a two-term sum exactly between two fp32 numbers, err = half an ulp;  column sums 0.89123
On a library built from the previous csrc/f32path.hip the NaN case of act 2 and 18 of the 42 pool-forward cases fail (the special draw
of every map but the 1 x 1 one, and the map [[1, nan, 3], [4, 5, nan], [0, 9, 2]]: 9 with index 7 where torch reports NaN with index
5); the rest passes.
"""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_UNSUPPORTED = -1, -3


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def run(case, what):
    """Allocate every buffer of the case between guards, make its calls, compare every buffer whole.  -> {buffer: window}"""
    call, sp, _ = _abi()
    bufs = {k: U.Guarded(b.size, kind, DEV, b) for k, (kind, b) in case.bufs.items()}
    for name, args in case.calls:
        a = [bufs[x.buf].ptr(x.off) if isinstance(x, R.P) else sp() if isinstance(x, str) else x for x in args]
        call(name, *a)
    torch.cuda.synchronize()
    got = {k: b.read()[0].copy() for k, b in bufs.items()}
    worst = max(w.ratio(got[k]) for k, w in case.want.items())
    if any(w.soft.any() for w in case.want.values()):
        print("F32-ERR %s: err / bound %.5f" % (what, worst))
    for k, w in case.want.items():
        assert w.ratio(got[k]) <= 1.0, (what, k, w.ratio(got[k]))
        win = bufs[k].check(w.hard_bits(got[k]), "%s: %s" % (what, k))
        if w.kind == "f32":                               # what must stay untouched holds the sentinel itself, not some other NaN
            keep = (w.bits == np.uint32(U.SENT32)) & ~w.soft
            assert bool(np.all(win[keep] == np.uint32(U.SENT32))), "%s: %s: an element outside the result was written" % (what, k)
    assert case.exact == (not any(w.soft.any() for w in case.want.values()))
    return got


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,shape,tr,acc,dr", R.CONV_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_conv(k, s, shape, tr, acc, dr):
    run(R.conv_case(k, s, shape, tr, acc, dr), "conv k%d s%d %s tr%d acc%d %s" % (k, s, shape, tr, acc, dr))


@pytest.mark.parametrize("dr", ["int", "normal"])
def test_conv_stem_form(dr):
    run(R.conv_stem_case(dr), "conv stem %s" % dr)


@pytest.mark.parametrize("dr", ["int", "normal"])
def test_conv_head_form(dr):
    got = run(R.conv_head_case(dr), "conv head %s" % dr)
    y = got["y"].reshape(2, R.HEAD_A, -1)
    assert bool(np.all(y[:, [0, R.HEAD_A - 1]] == np.uint32(U.SENT32))), "a row of no level was written"


@pytest.mark.parametrize("k,s,shape,dr", R.WGRAD_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_conv_wgrad(k, s, shape, dr):
    run(R.wgrad_case(k, s, shape, dr), "wgrad k%d s%d %s %s" % (k, s, shape, dr))


@pytest.mark.parametrize("M,C,act,dr", R.BN_PARAMS)
def test_bn_act_fwd(M, C, act, dr):
    run(R.bn_fwd_case(M, C, act, dr), "bn fwd M%d C%d act%d %s" % (M, C, act, dr))


@pytest.mark.parametrize("act", [0, 2, 3])
def test_bn_act_fwd_keeps_nan(act):
    """A NaN in z makes its channel's statistics, and with them every y of the channel, NaN - through the ReLU too (torch.relu keeps a
    NaN; fmaxf(u, 0) would report 0).  The other channels are bit for bit."""
    case = R.bn_fwd_case(256, 3, act, "exact", nan=True)
    got = run(case, "bn fwd NaN act%d" % act)
    y = U.from_bits32(got["y"]).reshape(256, -1)
    assert bool(np.all(np.isnan(y[:, 1]))) and not np.isnan(y[:, [0, 2]]).any()


@pytest.mark.parametrize("M,C,act,dr", R.BN_PARAMS)
def test_bn_act_bwd(M, C, act, dr):
    run(R.bn_bwd_case(M, C, act, dr), "bn bwd M%d C%d act%d %s" % (M, C, act, dr))


@pytest.mark.parametrize("shape,C,dr,layout", R.SPP_FWD_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_spp_fwd(shape, C, dr, layout):
    got = run(R.spp_fwd_case(shape, C, dr, layout), "spp fwd")
    if dr == "nan33":                                     # [[1, nan, 3], [4, 5, nan], [0, 9, 2]]: NaN with index 5 everywhere
        y, idx = U.from_bits32(got["y0"]).reshape(9, -1), got["idx"].reshape(3, 9, C)
        assert bool(np.all(np.isnan(y[:, 0]))) and bool(np.all(idx[:, :, 0] == 5))


@pytest.mark.parametrize("shape,C,dr,acc", R.SPP_BWD_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_spp_bwd(shape, C, dr, acc):
    run(R.spp_bwd_case(shape, C, dr, acc), "spp bwd %s C%d %s acc%d" % (shape, C, dr, acc))


def test_upsample2_fwd():
    run(R.up_fwd_case(), "upsample fwd")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dr", ["int", "normal"])
def test_upsample2_bwd(dr, acc):
    """bit for bit on normal draws too: the fp32 order is fixed"""
    run(R.up_bwd_case(dr, acc), "upsample bwd")


@pytest.mark.parametrize("mode", ["bits", "int", "normal"])
def test_rows_copy(mode):
    got = run(R.copy_case(mode), "rows_copy")
    if mode == "bits":                                    # NaN payloads too: the copy moves patterns
        want = R.copy_case(mode).want["dst"].bits
        assert np.array_equal(got["dst"], want)


@pytest.mark.parametrize("ld", R.STEM_LD)
@pytest.mark.parametrize("image", R.STEM_IMAGES, ids=str)
def test_stem_pack(image, ld):
    got = run(R.stem_case(image, ld), "stem_pack")
    assert not got["rows"].reshape(-1, ld)[:, 108:].any()


@pytest.mark.parametrize("C,with_origin", R.DEC_PARAMS)
def test_head_decode_bwd(C, with_origin):
    got = run(R.decode_case(C, with_origin), "decode bwd")
    assert not got["reg"].reshape(-1, 32)[:, 27:].any() and not got["cls"].reshape(-1, (C + 7) & ~7)[:, C:].any(), "a pad column is not +0"


@pytest.mark.parametrize("M,N,dr", R.COLSUM_PARAMS)
def test_colsum(M, N, dr):
    run(R.colsum_case(M, N, dr), "colsum M%d N%d %s" % (M, N, dr))


# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every EP24_REQUIRE of csrc/f32path.hip: the call returns its code and no buffer changes.  Every other argument of every call is
    valid, so nothing here could make a kernel act on a bad one."""
    _, sp, lib = _abi()
    bufs = {k: U.Guarded(n, kind, DEV) for k, (n, kind) in dict(
        a=(4096, "f32"), b=(4096, "f32"), c=(4096, "f32"), d=(4096, "f32"), e=(4096, "f32"), v=(64, "f32"), w=(64, "f32"), idx=(4096, "i32"),
        nbt=(1, "i64"), sums=(64, "f64")).items()}
    p = {k: b.ptr() for k, b in bufs.items()}
    st = sp()
    good = {
        "ep24_f32_stem_pack": [p["a"], p["b"], 112, 1, 4, 6, st],
        "ep24_f32_conv": [p["a"], 4, p["v"], 4, 4, p["b"], 4, 0, 0, p["w"], 0, 1, 4, 6, 4, 4, 1, 1, 0, st],
        "ep24_f32_conv_wgrad": [p["a"], 4, p["b"], 4, p["v"], 4, 4, 1, 4, 6, 4, 4, 1, 1, st],
        "ep24_f32_bn_act_fwd": [p["a"], 4, p["v"], p["w"], p["v"], p["w"], p["nbt"], p["w"], p["b"], 4, p["c"], 4, 24, 4, 1e-5, 0.125, 1, st],
        "ep24_f32_bn_act_bwd": [p["a"], 4, p["b"], 4, p["v"], p["v"], p["v"], p["sums"], p["w"], p["w"], p["c"], 4, 24, 4, 1, st],
        "ep24_f32_spp_fwd": [p["a"], 4, p["b"], p["c"], p["d"], 4, p["idx"], 1, 4, 6, 4, st],
        "ep24_f32_spp_bwd": [p["a"], p["b"], p["c"], 4, p["idx"], p["d"], 4, 0, 1, 4, 6, 4, st],
        "ep24_f32_upsample2_fwd": [p["a"], 4, p["b"], 4, 1, 4, 6, 4, st],
        "ep24_f32_upsample2_bwd": [p["a"], 4, p["b"], 4, 0, 1, 4, 6, 4, st],
        "ep24_f32_rows_copy": [p["a"], 4, p["b"], 4, 0, 24, 4, st],
        "ep24_f32_head_decode_bwd": [p["a"], p["b"], p["c"], p["d"], 1, 30, 2, 4, 6, 8.0, 30, p["e"], st],
        "ep24_f32_colsum": [p["a"], 32, p["v"], 24, 27, st],
    }
    bad = {
        "ep24_f32_stem_pack": [("images", None), ("rows", None), ("H", 5), ("W", 5), ("B", 0), ("ld", 107)],
        "ep24_f32_conv": [("x", None), ("w", None), ("y", None), ("B", 0), ("Cin", 0), ("Cout", 0), ("ksize", 2, E_UNSUPPORTED), ("ksize", 5, E_UNSUPPORTED),
                          ("stride", 0, E_UNSUPPORTED), ("stride", 3, E_UNSUPPORTED)],
        "ep24_f32_conv_wgrad": [("x", None), ("dy", None), ("dw", None)],
        "ep24_f32_bn_act_fwd": [("z", None), ("gamma", None), ("beta", None), ("save", None), ("y", None), ("M", 0), ("C", 0)],
        "ep24_f32_bn_act_bwd": [("dy", None), ("z", None), ("save", None), ("gamma", None), ("beta", None), ("sums", None), ("dz", None), ("M", 0), ("C", 0),
                                ("gamma_grad", None), ("beta_grad", None)],
        "ep24_f32_spp_fwd": [("x", None), ("y5", None), ("y9", None), ("y13", None), ("idx", None)],
        "ep24_f32_spp_bwd": [("dy5", None), ("dy9", None), ("dy13", None), ("idx", None), ("dx", None)],
        "ep24_f32_upsample2_fwd": [("x", None), ("y", None)],
        "ep24_f32_upsample2_bwd": [("dy", None), ("dx", None)],
        "ep24_f32_rows_copy": [("src", None), ("dst", None)],
        "ep24_f32_head_decode_bwd": [("dout", None), ("out", None), ("d_regobj", None), ("d_cls", None), ("ncols", 27)],
        "ep24_f32_colsum": [("g", None), ("db", None), ("N", 0)],
    }
    wrong = []

    def calls():                                          # on a thread of their own: the last-error text is per thread, and tests of
        for name, args in good.items():                   # other files expect this thread's to stay empty
            names = [a for _, a in lib.protos[name][1]]
            assert len(names) == len(args), name
            for key, val, *code in bad[name]:
                a = list(args)
                a[names.index(key)] = val
                wrong.append((name, key, val, lib.fn[name](*a), code[0] if code else E_ARG))
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert len(wrong) == sum(len(v) for v in bad.values()) == 61
    assert not [w for w in wrong if w[3] != w[4]], [w for w in wrong if w[3] != w[4]]
    torch.cuda.synchronize()
    for k, b in bufs.items():
        b.check(np.full(b.n, b.sent, dtype=b.host.dtype), k)
