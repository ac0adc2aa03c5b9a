"""GPU: the conv forward and data-gradient kernels stage by stage against the fp64 oracles of tests/conv_oracles.py.

The launchers are called directly (``_lib.call``), so every stored tensor is in the test's hands: each stage is
compared per element with fp64 from the tensors the kernel itself stored or was given for the stage before.  No
tolerance is a constant: 16 x the measured error of an fp32 torch evaluation of the same stage, half a bf16 ulp for
a bf16 store, the documented 1.5e-7 of the A&S erf core in the exact build, and for the two roundings the kernels
never store (``pre + bias`` in the forward, dS1 in ``pbx_conv_dgrad4f``) an admissible interval whose width -- zero
for ~98 % of the elements -- is carried into the stages behind it.  ``dpre = bf16(ds1 * gd)`` and the fragment
packer are bitwise.  tests/test_conv_oracles.py shows on the CPU that the oracle is right and that these conditions
reject eight kinds of wrong kernel.

Every output has 16 guard rows filled with a NaN sentinel (``test_hip_global_exact.Buf``): guards must stay
untouched, no sentinel may remain below, and a second launch repeats bitwise.  ``PBX_CONV_EXACT_REPORT=path``
writes each tensor's largest err / e32 over the session, the ambiguous shares and the M2 ratios
(profiles/r22/conv_exact.txt)."""
import contextlib
import os

import pytest
import torch

import conv_oracles as co
from conv_oracles import BM, C, DIL, EPS, KS, V
from test_hip_global_exact import Buf

from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.ops import local_track as lt

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
LEDGER = co.ConvLedger()


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    out = os.environ.get("PBX_CONV_EXACT_REPORT")
    if out and LEDGER.worst:
        with open(out, "w") as fh:
            fh.write("largest err / e32 per checked tensor over all cases of tests/test_hip_conv_exact.py\n"
                     "(assertion: err <= 16 e32 beyond the free terms; bf16 rows: excess over the half ulp)\n")
            for n, r in LEDGER.worst.items():
                fh.write(f"{n:<34s} {r:8.3f}\n")
            fh.write("\nlargest ambiguous shares, e32 of the hidden roundings and M2 ratios\n")
            for n, r in LEDGER.notes.items():
                fh.write(f"{n:<44s} {r:10.4g}\n")


def _dev():
    return torch.device("cuda")


def _st():
    return _lib.stream_ptr(_dev())


def _to_dev(c):
    return {n: (v.to(_dev()) if torch.is_tensor(v) else v) for n, v in c.items()}


def _packs(cd):
    (wpn, wtn), (wpw, wtw) = lt.pack_conv(cd["wn"]), lt.pack_conv(cd["ww"])
    return dict(wpn=wpn, wtn=wtn, wpw=wpw, wtw=wtw)


def _rows(buf, B, L):
    """[B, L, C] view of a [B L (+ guard), C] buffer, on the CPU."""
    return buf.v.detach().cpu().reshape(B, L, C).clone()


def _written(bufs):
    for n, b in bufs.items():
        if b is not None:
            b.assert_written(n)


def _same_bits(a, b, names):
    for n in names:
        if a.get(n) is not None:
            it = torch.int16 if a[n].dt == BF16 else torch.int32
            assert torch.equal(a[n].v.view(it), b[n].v.view(it)), f"{n}: two launches differ"


@contextlib.contextmanager
def exact_library():
    """The exact-GELU build loaded beside the session's library, and the session's mode restored afterwards
    (``_lib.set_gelu`` refuses once a library is loaded, so the loaded one is set aside for the duration)."""
    saved = (_lib.HIP_LIB, _lib._lib, dict(_lib._FN), os.environ.get("PBX_GELU"))
    _lib._lib = None
    _lib._FN.clear()
    try:
        _lib.set_gelu("exact")
        assert _lib.gelu_mode() == "exact"
        yield
    finally:
        torch.cuda.synchronize()
        _lib.HIP_LIB, _lib._lib = saved[0], saved[1]
        _lib._FN.clear()
        _lib._FN.update(saved[2])
        if saved[3] is None:
            os.environ.pop("PBX_GELU", None)
        else:
            os.environ["PBX_GELU"] = saved[3]


# ---- forward ------------------------------------------------------------------------------------------------
FWD_X = ("pbx_conv_fwd3x", "pbx_conv_fwd5x")


def launch_fwd(name, cd, pk, store=True):
    """One forward launcher into fresh sentinel-filled buffers.  Returns (bufs, stats tensor, layout)."""
    B, L, lo, hi = cd["B"], cd["L"], cd["lo"], cd["hi"]
    T = (L + BM - 1) // BM
    b = dict(gdn=Buf(B * L, C, dt=BF16) if store else None, gdw=Buf(B * L, C, dt=BF16) if store else None,
             s1=Buf(B * L, C, dt=BF16), stats=Buf(B * T, 2))
    P = lambda n: None if b[n] is None else b[n].full.data_ptr()  # noqa: E731
    layout = ("rows", BM)
    if name in FWD_X:
        _lib.call(name, cd["x"].data_ptr(), pk["wpn"].data_ptr(), pk["wpw"].data_ptr(), cd["bn"].data_ptr(),
                  cd["bw"].data_ptr(), cd["gb"].data_ptr(), P("gdn"), P("gdw"), P("s1"), P("stats"), B, L, KS, DIL,
                  lo, hi, _st())
    elif name == "pbx_conv_fwd3t":
        _lib.call(name, cd["tok"].data_ptr(), cd["emb"].data_ptr(), pk["wpn"].data_ptr(), pk["wpw"].data_ptr(),
                  cd["bn"].data_ptr(), cd["bw"].data_ptr(), cd["gb"].data_ptr(), P("gdn"), P("gdw"), P("s1"),
                  P("stats"), B, L, KS, DIL, _st())
    else:                       # lt.conv_fwd_first: pbx_conv_tok_tables + pbx_conv_fwd_tok, or pbx_conv_fwd3t
        f = lambda n: None if b[n] is None else b[n].full  # noqa: E731
        st1, T1, bm1 = lt.conv_fwd_first(cd["tok"], cd["emb"], pk["wpn"], pk["wpw"], cd["bn"], cd["bw"], cd["gb"],
                                         f("gdn"), f("gdw"), f("s1"), KS, DIL, _st())
        b["stats"] = None
        torch.cuda.synchronize()
        assert st1.shape == (B, T1, 2) and bool(torch.isfinite(st1).all()), "stats: not every partial written"
        return b, st1.detach().cpu(), (("tok",) if bm1 == 4 else ("rows", bm1))
    torch.cuda.synchronize()
    return b, b["stats"].v.detach().cpu().reshape(B, T, 2).clone(), layout


def _k_of(b, stats, B, L):
    return dict(gdn=None if b["gdn"] is None else _rows(b["gdn"], B, L),
                gdw=None if b["gdw"] is None else _rows(b["gdw"], B, L), s1=_rows(b["s1"], B, L), stats=stats)


def _forward_case(B, L, lo=0, hi=0, shift=0.0, names=FWD_X, expect_tok=None):
    """Every launcher of ``names`` on one case: STORE form (twice: bitwise), inference form, all against one
    reference."""
    mode = _lib.gelu_mode()
    assert mode in ("fitted", "exact")
    c = co.make_case(B, L, lo, hi, gb_shift=shift, tok=not (lo or hi))
    cd = _to_dev(c)
    pk = _packs(cd)
    tag = "fwd|halo" if lo or hi else "fwd"
    ref = co.forward_ref(c, mode, LEDGER, None, tag)
    for name in names:
        print(f"-- {name} ({mode})")
        b, stats, layout = launch_fwd(name, cd, pk)
        if name == "first" and expect_tok is not None:
            assert (layout == ("tok",)) == expect_tok and lt.conv_tok_ok(B, L, KS, DIL, V) == expect_tok
        _written(b)
        sub = tag + ("|tok" if layout == ("tok",) else "")
        k = _k_of(b, stats, B, L)
        co.check_forward(c, k, mode, layout, LEDGER, None, sub, ref)
        b2, stats2, _ = launch_fwd(name, cd, pk)
        _same_bits(b, b2, ("gdn", "gdw", "s1", "stats"))
        assert torch.equal(stats, stats2), "stats: two launches differ"
        # the inference form: s1 and the partials written, no GELU' buffer to touch (the launchers select it by
        # null pointers, so none can be passed).  Bitwise equal to the checked training form, or (the erf core
        # evaluates GELU alone in another form) checked on its own
        bi, statsi, _ = launch_fwd(name, cd, pk, store=False)
        _written(bi)
        ki = _k_of(bi, statsi, B, L)
        if not (torch.equal(ki["s1"].view(torch.int16), k["s1"].view(torch.int16)) and torch.equal(statsi, stats)):
            co.check_forward(c, ki, mode, layout, LEDGER, None, sub + "|inf", ref)
    return c, cd, pk


ALL4 = FWD_X + ("pbx_conv_fwd3t", "first")
# (B, L, gb shift, the token kernel takes the shape): one tile with both halos of both convs outside; a second
# tile of 2 rows (gb + 3: the one-pass M2 term); odd L, a last tile of 1 row; full tiles, the dilation-5 taps
# across a tile boundary; a grid of one; 261 tiles on 256 workgroups (conv_fwd5's second round starts mid-sample,
# a grid tail); 516 tiles, a third round; the token form's wrap; L = 200, which the token form declines
FWD_CASES = [(2, 36, 0.0, False), (3, 130, 3.0, False), (2, 257, 0.0, False), (3, 256, 0.0, True),
             (1, 128, 0.0, True), (87, 300, 0.0, False), (172, 300, 0.0, False), (40, 512, 0.0, True),
             (2, 200, 0.0, False)]


@pytest.mark.parametrize("B,L,shift,tok_ok", FWD_CASES)
def test_forward_stagewise(B, L, shift, tok_ok):
    """pbx_conv_fwd3x, pbx_conv_fwd5x, pbx_conv_fwd3t and lt.conv_fwd_first (pbx_conv_tok_tables + pbx_conv_fwd_tok
    where it takes the shape, else the pbx_conv_fwd3t fallback) on x = emb[tok]: GELU' images, s1 and the
    LayerNorm partials per element against the oracle."""
    _forward_case(B, L, shift=shift, names=ALL4, expect_tok=tok_ok)


@pytest.mark.parametrize("B,L", [(3, 256), (2, 300)])
def test_forward_halo_rows(B, L):
    """xlo = xhi = 20 non-zero neighbour rows (the context-parallel call) against the direct definition."""
    _forward_case(B, L, 20, 20)


@pytest.mark.parametrize("B,L", [(2, 257), (3, 256)])
def test_forward_exact_library(B, L):
    """The same sources built with the A&S erf core: the oracle's erf form plus the core's documented 1.5e-7."""
    with exact_library():
        _forward_case(B, L, names=ALL4, expect_tok=L % BM == 0)
    assert _lib.gelu_mode() != "custom"


def test_token_tables_and_packer():
    """pbx_pack_conv_frag: both images bitwise against the index formula above pack_conv_frag_kernel.
    pbx_conv_tok_tables: T[half][conv][tap][v][co] = sum_ci bf16(W[co, ci, tap]) emb[v, ci], row V zero."""
    c = co.make_case(1, 128, tok=True)
    cd = _to_dev(c)
    idx = torch.arange(KS * C * C)
    j, lane, fi = idx & 7, (idx >> 3) & 63, idx >> 9
    mb, kb, k = fi & 3, (fi >> 2) & 7, fi >> 5
    m, kk = mb * 32 + (lane & 31), kb * 16 + 8 * (lane >> 5) + j
    for w in ("wn", "ww"):
        pf, pt = Buf(KS * C, C, dt=BF16), Buf(KS * C, C, dt=BF16)
        _lib.call("pbx_pack_conv_frag", cd[w].data_ptr(), pf.full.data_ptr(), pt.full.data_ptr(), KS, _st())
        torch.cuda.synchronize()
        pf.assert_written("forward image")
        pt.assert_written("dgrad image")
        wb = co.rne_bf16(c[w])
        co.check_bits(f"pack.{w}.fwd", pf.v.cpu().reshape(-1), wb[m, kk, k])       # M = co, K = ci
        co.check_bits(f"pack.{w}.dgrad", pt.v.cpu().reshape(-1), wb[kk, m, k])     # M = ci, K = co
    pk = _packs(cd)
    tab = lt.conv_tok_tables(pk["wpn"], pk["wpw"], cd["emb"])
    torch.cuda.synchronize()
    tab = tab.cpu()
    assert tab.shape == (2, 2, KS, V + 1, C // 2) and bool((tab[:, :, :, V] == 0).all())
    for ci, w in enumerate(("wn", "ww")):
        t64, t32 = [torch.einsum("ock,vc->kvo", co.rne_bf16(c[w]).to(dt), c["emb"].to(dt)) for dt in (F64, F32)]
        got = torch.cat([tab[0, ci, :, :V], tab[1, ci, :, :V]], dim=-1)              # [tap, v, 128]
        co.check_elem(f"tok_tables.{w}", got, t64, co._e32(t32, t64), None, LEDGER)


# ---- backward -----------------------------------------------------------------------------------------------
BWD_CASES = [(2, 36), (3, 130), (2, 257), (2, 512)]


def launch_dgrad4x(cd, pk, gdn, gdw, ds1):
    B, L = cd["B"], cd["L"]
    b = dict(dx=Buf(B * L, C, dt=BF16), dpn=Buf(B * L, C, dt=BF16), dpw=Buf(B * L, C, dt=BF16))
    _lib.call("pbx_conv_dgrad4x", ds1.data_ptr(), gdn.data_ptr(), gdw.data_ptr(), pk["wtn"].data_ptr(),
              pk["wtw"].data_ptr(), b["dx"].full.data_ptr(), b["dpn"].full.data_ptr(), b["dpw"].full.data_ptr(),
              B, L, KS, DIL, cd["lo"], cd["hi"], _st())
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("B,L,H", [(b, l, 0) for b, l in BWD_CASES] + [(3, 256, 20), (2, 300, 20)])
def test_dgrad4x(B, L, H):
    """pbx_conv_dgrad4x on random dS1 and GELU' rows (H: ilo = ihi = 20 neighbour rows): dpre bitwise, dx from the
    stored dpre rows and the halo rows' exact products."""
    c = co.make_case(B, L, H, H)
    cd = _to_dev(c)
    pk = _packs(cd)
    b = launch_dgrad4x(cd, pk, cd["gdn"], cd["gdw"], cd["ds1"])
    _written(b)
    got = {n: _rows(v, B, L) for n, v in b.items()}
    co.check_dgrad(c, c["gdn"], c["gdw"], got, LEDGER, None, "dgrad4x|halo" if H else "dgrad4x")
    _same_bits(b, launch_dgrad4x(cd, pk, cd["gdn"], cd["gdw"], cd["ds1"]), ("dx", "dpn", "dpw"))


def _forward_state(B, L, bm1=BM, ts1=None):
    """The training forward (pbx_conv_fwd3x) of one case and the LayerNorm-1 tables of its stored s1: st1 the
    kernel's own partials (``bm1`` = 128) or synthetic ones of ``bm1`` rows, sums1 built here in fp64."""
    c = co.make_case(B, L)
    cd = _to_dev(c)
    pk = _packs(cd)
    fb, stats, _ = launch_fwd("pbx_conv_fwd3x", cd, pk)
    k = _k_of(fb, stats, B, L)
    if bm1 != BM:
        m, M2, _ = co.st_stats(k["s1"], L, ("rows", bm1), F64)
        k["st1"] = torch.stack([m, M2], dim=-1).to(F32)
    else:
        k["st1"] = stats
    ts1 = ts1 or (L + 1) // 2
    k["sums1"] = co.make_sums1(c["dh1"], k["s1"], c["g1"], k["st1"], bm1, L, ts1)
    kd = {n: k[n].to(_dev()).contiguous() for n in ("s1", "st1", "sums1", "gdn", "gdw")}
    return c, cd, pk, k, kd, ts1


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("B,L", BWD_CASES)
def test_ln1_finalize(B, L, det):
    """pbx_ln1_finalize: the stored dS1 inside its admissible interval, dgb (preloaded) against the column sums of
    the stored dS1; ``det``: one workgroup per sample walks every tile, so dgb repeats bitwise."""
    c, cd, pk, k, kd, ts1 = _forward_state(B, L)
    T1 = k["st1"].shape[1]

    def launch():
        b = dict(ds1=Buf(B * L, C, dt=BF16), dgb=Buf(B, C, fill=cd["dgb0"]))
        _lib.call("pbx_ln1_finalize", cd["dh1"].data_ptr(), kd["s1"].data_ptr(), kd["st1"].data_ptr(), T1, BM,
                  kd["sums1"].data_ptr(), ts1, cd["g1"].data_ptr(), b["ds1"].full.data_ptr(),
                  b["dgb"].full.data_ptr(), B, L, EPS, det, _st())
        torch.cuda.synchronize()
        return b

    b = launch()
    _written(b)
    got = dict(ds1=_rows(b["ds1"], B, L), dgb=b["dgb"].v.cpu().clone())
    co.check_ln1(c, k, got, BM, EPS, LEDGER, None, "ln1|det" if det else "ln1")
    _same_bits(b, launch(), ("ds1", "dgb") if det else ("ds1",))


def _dgrad4f(B, L, bm1, ts1, tag):
    c, cd, pk, k, kd, ts1 = _forward_state(B, L, bm1, ts1)
    T1 = k["st1"].shape[1]

    def launch():
        b = dict(dx=Buf(B * L, C, dt=BF16), dpn=Buf(B * L, C, dt=BF16), dpw=Buf(B * L, C, dt=BF16),
                 dgb=Buf(B, C, fill=cd["dgb0"]))
        _lib.call("pbx_conv_dgrad4f", cd["dh1"].data_ptr(), kd["s1"].data_ptr(), kd["st1"].data_ptr(), T1, bm1,
                  kd["sums1"].data_ptr(), ts1, cd["g1"].data_ptr(), kd["gdn"].data_ptr(), kd["gdw"].data_ptr(),
                  pk["wtn"].data_ptr(), pk["wtw"].data_ptr(), b["dx"].full.data_ptr(), b["dpn"].full.data_ptr(),
                  b["dpw"].full.data_ptr(), b["dgb"].full.data_ptr(), B, L, KS, DIL, EPS, _st())
        torch.cuda.synchronize()
        return b

    b = launch()
    _written(b)
    got = {n: _rows(b[n], B, L) for n in ("dx", "dpn", "dpw")}
    got["dgb"] = b["dgb"].v.cpu().clone()
    co.check_dgrad_fin(c, k, bm1, got, EPS, LEDGER, None, tag)
    # dgb: one float atomic per tile onto the preloaded value, so it repeats bitwise with a single tile only
    _same_bits(b, launch(), ("dx", "dpn", "dpw", "dgb") if L <= BM else ("dx", "dpn", "dpw"))


@pytest.mark.parametrize("B,L", BWD_CASES)
def test_dgrad4f(B, L):
    """pbx_conv_dgrad4f from the forward kernel's own s1, partials and GELU' images: dS1 is never stored, so dpre,
    dx and dgb are evaluated at the low end of its admissible interval and gain |gd| gap, gap and sum gap."""
    _dgrad4f(B, L, BM, None, "dgrad4f")


def test_dgrad4f_long_partial_tables():
    """(BM1, T1, TS1) = (2, 129, 600) at L = 257: the second trips of wave_ln_stats_from (T > 64) and of
    wave_bwd_consts_from<8> (T > 512) in mfma.h, which no workload shape below L = 8192 / 16384 enters."""
    _dgrad4f(2, 257, 2, 600, "dgrad4f|synthetic")


@pytest.mark.parametrize("slab", [False, True])
def test_embed_dpre(slab):
    """pbx_embed_dpre, atomic and slab form, at 3 x 300 rows (two workgroups of two tiles, the last one partial):
    dpn / dpw bitwise, dE (preloaded) against the fp64 index_add of dS1."""
    B, L = 3, 300
    c = co.make_case(B, L, tok=True)
    cd = _to_dev(c)
    groups = _lib.lib().pbx_embed_bwd_groups(B * L)
    assert groups == 2

    def launch():
        b = dict(dpn=Buf(B * L, C, dt=BF16), dpw=Buf(B * L, C, dt=BF16), dE=Buf(V, C, fill=cd["dE0"]))
        sl = torch.full((groups, V, C), float("nan"), device=_dev()) if slab else None
        _lib.call("pbx_embed_dpre", cd["tok"].data_ptr(), cd["ds1"].data_ptr(), cd["gdn"].data_ptr(),
                  cd["gdw"].data_ptr(), b["dpn"].full.data_ptr(), b["dpw"].full.data_ptr(), b["dE"].full.data_ptr(),
                  B * L, V, _lib.ptr(sl), _st())
        torch.cuda.synchronize()
        return b

    b = launch()
    _written(b)
    got = dict(dpn=_rows(b["dpn"], B, L), dpw=_rows(b["dpw"], B, L), dE=b["dE"].v.cpu().clone())
    co.check_embed_dpre(c, c["ds1"], c["gdn"], c["gdw"], got, LEDGER, None, "embed_dpre|slab" if slab else "embed_dpre")
    _same_bits(b, launch(), ("dpn", "dpw", "dE") if slab else ("dpn", "dpw"))
