"""GPU: the global-track kernels stage by stage against the fp64 oracles of tests/global_oracles.py.

The launchers are called directly (``_lib.call`` with ``global_track._ptrs``), so every stored intermediate is
in the test's hands: each stage is compared with fp64 from the kernel's own stored inputs to that stage, and the
only legitimate error is fp32 arithmetic.  No tolerance here is a constant: each is 16 x the measured error of
an fp32 torch evaluation of the same stage, plus (where a GELU / GELU' is applied) the documented 1.5e-7 of the
A&S erf core times the magnitude it multiplies, plus (bf16 stores) half a bf16 ulp.  tests/test_global_oracles.py
shows on the CPU that the oracle is right and that these conditions reject six kinds of wrong kernel.

Every output is allocated with 16 guard rows past B and filled with a sentinel (NaN; a NaN bit pattern for
bf16): guards must stay untouched and no sentinel may remain in the rows < B.  ``PBX_GLOBAL_EXACT_REPORT=path``
writes each tensor's largest err / e32 over the session (profiles/r20/global_track_exact.txt)."""
import os

import pytest
import torch

import global_oracles as go
from global_oracles import EPS, make_case

from proteinbert_pytorch_replication_amd.ops import _lib, global_track as gt
from proteinbert_pytorch_replication_amd.utils import determinism

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
GUARD = 16
BF_SENTINEL = 0x7FA5          # a bf16 NaN bit pattern
LEDGER = go.Ledger()
SUMS = go.BWD_SUMS


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    out = os.environ.get("PBX_GLOBAL_EXACT_REPORT")
    if out and LEDGER.worst:
        with open(out, "w") as fh:
            fh.write("largest err / e32 per checked tensor over all cases of tests/test_hip_global_exact.py\n"
                     "(assertion: err <= 16 e32 + GELU core term; bf16 rows: excess over the half ulp)\n")
            for n, r in LEDGER.worst.items():
                fh.write(f"{n:<22s} {r:8.3f}\n")


def _dev():
    return torch.device("cuda")


def _st():
    return _lib.stream_ptr(_dev())


class Buf:
    """An output with guard rows: ``full`` [(rows + 16), ...] sentinel-filled, ``v`` the first ``rows``."""

    def __init__(self, rows, *cols, dt=F32, fill=None):
        self.rows, self.dt = rows, dt
        self.full = torch.empty((rows + GUARD, *cols), dtype=dt, device=_dev())
        self._sentinel(self.full)
        self.v = self.full[:rows]
        if fill is not None:
            self.v.copy_(fill)

    @staticmethod
    def _sentinel(t):
        if t.dtype == BF16:
            t.view(torch.int16).fill_(BF_SENTINEL)
        else:
            t.fill_(float("nan"))

    def guards_ok(self):
        t = self.full[self.rows:]
        return bool((t.view(torch.int16) == BF_SENTINEL).all()) if self.dt == BF16 else bool(torch.isnan(t).all())

    def untouched(self):
        t = self.full
        return bool((t.view(torch.int16) == BF_SENTINEL).all()) if self.dt == BF16 else bool(torch.isnan(t).all())

    def assert_written(self, name):
        assert self.guards_ok(), f"{name}: rows >= B were written"
        assert bool(torch.isfinite(self.v.float()).all()), f"{name}: a sentinel remains in the rows < B"


def _to(d, dev):
    return {n: (None if v is None else v.to(dev)) for n, v in d.items()}


def _cpu(bufs):
    return {n: (None if b is None else b.v.detach().cpu().clone()) for n, b in bufs.items()}


def _packs(par):
    f1, f1T = gt.pack_glob(par["w1"])
    f2, f2T = gt.pack_glob(par["w2"])
    fgl, fglT = gt.pack_glob(par["wgl"]) if par["wgl"] is not None else (None, None)
    return dict(f1=f1, f1T=f1T, f2=f2, f2T=f2T, fgl=fgl, fglT=fglT)


def launch_fwd(inp, par, pk, B, G, NGL, TV, K, bufs=None):
    """pbx_glob3_fwd into fresh sentinel-filled buffers (device tensors in ``inp`` / ``par``)."""
    NCT = G // 64
    b = bufs or dict(
        pre1=Buf(B, G), xh1=Buf(B, G), r1=Buf(B), vsum=Buf(B, G), g1_bf=Buf(B, G, dt=BF16), pre2=Buf(B, G),
        xh2=Buf(B, G), r2=Buf(B), g2=Buf(B, G), g2_bf=Buf(B, G, dt=BF16),
        pregl=Buf(B, NGL) if NGL else None, gb=Buf(B, NGL) if NGL else None, z1=Buf(B, G), z2=Buf(B, G),
        part1=Buf(B, NCT, 2), part2=Buf(B, NCT, 2))
    f = lambda n: None if b[n] is None else b[n].full  # noqa: E731
    _lib.call("pbx_glob3_fwd", gt._ptrs(inp["g"], inp["g_bf"], inp["vpart"], inp["wp"], pk["f1"], par["b1"],
                                        par["n1w"], par["n1b"], pk["f2"], par["b2"], par["n2w"], par["n2b"],
                                        pk["fgl"], par["bgl"], f("pre1"), f("xh1"), f("r1"), f("vsum"), f("g1_bf"),
                                        f("pre2"), f("xh2"), f("r2"), f("g2"), f("g2_bf"), f("pregl"), f("gb"),
                                        f("z1"), f("z2"), f("part1"), f("part2")),
              B, G, NGL, TV, K, EPS, _st())
    torch.cuda.synchronize()
    return b


def launch_bwd(dg2, dgb, kd, par, wp, pk, B, G, NGL, K, slab, pre, bufs=None, slab_rows=None):
    """pbx_glob_bwd; kd: device tensors the forward stored.  ``pre``: name -> preloaded column-sum values."""
    b = bufs or dict(dg=Buf(B, G), dvs=Buf(B, G), du1=Buf(B, G, dt=BF16), du2=Buf(B, G, dt=BF16),
                     dugl=Buf(B, NGL, dt=BF16) if NGL else None)
    if bufs is None:
        for n in SUMS:
            b[n] = None if pre.get(n) is None else Buf(pre[n].numel(), fill=pre[n])
    f = lambda n: None if b.get(n) is None else b[n].full  # noqa: E731
    sl = None
    if slab:
        sl = torch.full((slab_rows or (B + 15) // 16, 6 * G + NGL + K), float("nan"), dtype=F32, device=_dev())
    _lib.call("pbx_glob_bwd", gt._ptrs(dg2, dgb, kd.get("pregl"), pk["fglT"], kd["xh2"], kd["r2"], par["n2w"],
                                       kd["pre2"], pk["f2T"], kd["xh1"], kd["r1"], par["n1w"], kd["pre1"],
                                       kd["vsum"], wp, pk["f1T"], f("dg"), f("dvs"), f("du1"), f("du2"), f("dugl"),
                                       f("db1"), f("dn1w"), f("dn1b"), f("db2"), f("dn2w"), f("dn2b"), f("dbgl"),
                                       f("dwp")),
              B, G, NGL, K, _lib.ptr(sl), _st())
    torch.cuda.synchronize()
    return b


def _fwd_case(B, G, NGL, TV, K, off=False, seed=5):
    inp, par, dg2, dgb = make_case(B, G, NGL, TV, K, tile_offset=off, seed=seed)
    dev = _dev()
    return (inp, par, dg2, dgb), (_to(inp, dev), _to(par, dev), dg2.to(dev), None if dgb is None else dgb.to(dev))


def _equal_bufs(a, b):
    for n in a:
        if a[n] is not None:
            assert torch.equal(a[n].v.view(torch.int16 if a[n].dt == BF16 else torch.int32),
                               b[n].v.view(torch.int16 if b[n].dt == BF16 else torch.int32)), f"{n}: runs differ"


# (B, G, NGL) x TV x K: every value of each group; B = 17 and B = 37 with every TV and every K
FWD_CASES = [(1, 256, 0, 1, 64, False), (16, 256, 128, 4, 1, False),
             (17, 512, 128, 1, 1, False), (17, 512, 128, 3, 48, False), (17, 512, 128, 4, 64, False),
             (17, 512, 128, 5, 100, False), (17, 512, 128, 16, 48, False),
             (37, 512, 0, 1, 100, False), (37, 512, 0, 3, 64, False), (37, 512, 128, 4, 48, False),
             (37, 512, 128, 5, 1, False), (37, 512, 0, 16, 100, False), (37, 512, 128, 16, 64, False),
             (37, 512, 128, 5, 64, True), (17, 512, 128, 3, 100, True)]


@pytest.mark.parametrize("B,G,NGL,TV,K,off", FWD_CASES)
def test_fused_forward_stagewise(B, G, NGL, TV, K, off):
    """pbx_glob3_fwd: every stored tensor against its stage oracle (``off``: 3 x tile index added to g, so the
    between-tile term dominates the row variance and the Chan merge is what is tested); guards; twice bitwise."""
    (inp, par, _, _), (inp_d, par_d, _, _) = _fwd_case(B, G, NGL, TV, K, off)
    pk = _packs(par_d)
    b = launch_fwd(inp_d, par_d, pk, B, G, NGL, TV, K)
    for n, buf in b.items():
        if buf is not None:
            buf.assert_written(n)
    go.check_forward(inp, par, _cpu(b), EPS, LEDGER)
    _equal_bufs(b, launch_fwd(inp_d, par_d, pk, B, G, NGL, TV, K))


BWD_CASES = [(1, 256, 0, 512), (16, 256, 128, 1), (17, 512, 128, 48), (37, 512, 0, 64), (37, 512, 128, 100),
             (17, 512, 128, 512), (300, 256, 128, 64)]
BWD_OUT = ("dugl", "du2", "du1", "dg", "dvs") + SUMS


def _bwd_setup(B, G, NGL, K, TV=3):
    (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d) = _fwd_case(B, G, NGL, TV, K)
    pk = _packs(par_d)
    fb = launch_fwd(inp_d, par_d, pk, B, G, NGL, TV, K)
    kd = {n: (None if v is None else v.v) for n, v in fb.items()}
    k = _cpu(fb)
    k["g_bf"] = inp["g_bf"]
    gen = torch.Generator().manual_seed(11)
    pre = {n: torch.randn(s, generator=gen) for n, s in
           [("db1", G), ("dn1w", G), ("dn1b", G), ("db2", G), ("dn2w", G), ("dn2b", G), ("dwp", K)]}
    pre["dbgl"] = torch.randn(NGL, generator=gen) if NGL else None
    return (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d), pk, kd, k, pre


def _check_bwd_bufs(b, names):
    for n in names:
        if b.get(n) is not None:
            b[n].assert_written(n)


@pytest.mark.parametrize("B,G,NGL,K", BWD_CASES)
def test_fused_backward_both_forms(B, G, NGL, K):
    """pbx_glob_bwd from the tensors the forward launch stored, float-atomic form and slab form, both adding
    onto preloaded column-sum destinations; B = 300: 19 slab rows, the last tile partial."""
    (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d), pk, kd, k, pre = _bwd_setup(B, G, NGL, K)
    names = [n for n in BWD_OUT if NGL or n not in ("dugl", "dbgl")]
    res = {}
    for form in ("atomic", "slab", "slab2"):
        b = launch_bwd(dg2_d, dgb_d, kd, par_d, inp_d["wp"], pk, B, G, NGL, K, form != "atomic", pre)
        _check_bwd_bufs(b, names)
        res[form] = got = _cpu(b)
        if form != "slab2":
            print(f"-- {form}")
            o64, e32s = go.check_backward(dg2, dgb, k, par, inp["wp"], got, LEDGER, names, pre)
    for n in names:                                                       # slab form twice: bitwise
        assert torch.equal(res["slab"][n].float(), res["slab2"][n].float()), f"{n}: slab runs differ"
    for n in ("dg", "dvs", "du1", "du2", "dugl"):                       # independent of the reduction form
        if n in names:
            assert torch.equal(res["slab"][n].float(), res["atomic"][n].float()), f"{n}: slab vs atomic differ"
    for n in SUMS:                                     # slab against atomic: within the helper's bound of that sum
        if n in names:
            go.check(n + "|forms", res["slab"][n], res["atomic"][n], None, o64.get("_mag_" + n, 0.0), LEDGER,
                     e32=e32s[n])


def _unpermute(img, N, K, fwd):
    """The [N, K] matrix a fragment image holds, by the index formulas above pack_glob_frags_kernel."""
    idx = torch.arange(N * K)
    j, lane, f = idx & 7, (idx >> 3) & 63, idx >> 9
    if fwd:
        S = K // 32
        t, s = f // S, f % S
        row, col = t * 16 + (lane & 15), s * 32 + 8 * (lane >> 4) + j
    else:
        S = N // 32
        t, s = f // S, f % S
        row, col = s * 32 + 8 * (lane >> 4) + j, t * 16 + (lane & 15)
    out = torch.full((N, K), BF_SENTINEL, dtype=torch.int16)
    out[row, col] = img.cpu().view(torch.int16)
    return out


@pytest.mark.parametrize("N,K", [(128, 256), (256, 256), (512, 512), (128, 512)])
def test_pack_frags_exact(N, K):
    """pbx_pack_glob_frags and pbx_pack_batch kind 1: both images un-permuted equal the RNE bf16 of w exactly,
    and the two launchers agree bitwise."""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * K ** -0.5
    wd = w.to(_dev())
    ff, fb = gt.pack_glob(wd)
    o1 = torch.empty(N * K, dtype=BF16, device=_dev())
    o2 = torch.empty_like(o1)
    for t in (o1, o2):
        t.view(torch.int16).fill_(BF_SENTINEL)
    gt.pack_batch([(1, wd, o1, o2, N, K)])
    torch.cuda.synchronize()
    want = go.rne_bf16(w).view(torch.int16)
    assert torch.equal(_unpermute(ff, N, K, True), want), "forward image"
    assert torch.equal(_unpermute(fb, N, K, False), want), "backward image"
    assert torch.equal(ff.view(torch.int16), o1.view(torch.int16)) and torch.equal(fb.view(torch.int16),
                                                                                 o2.view(torch.int16))


# ---- the general path (glob.hip) ----------------------------------------------------------------------
def _row_inputs(B, G, TV, K, seed=3):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc  # noqa: E731
    return dict(u=rn(B, G), bias=rn(G, sc=0.1), res=rn(B, G), vpart=rn(B, TV, G, sc=0.05), wp=rn(K),
                nw=1 + rn(G, sc=0.1), nb=rn(G, sc=0.1), dout=rn(B, G))


@pytest.mark.parametrize("B,G,TV,K,att", [(1, 100, 1, 1, True), (1, 100, 5, 48, False), (37, 384, 5, 48, True),
                                          (37, 384, 1, 256, True), (37, 384, 1, 1, False), (5, 1024, 5, 256, True),
                                          (5, 1024, 1, 48, False)])
def test_row_ln_kernels(B, G, TV, K, att):
    """pbx_row_ln_fwd / pbx_row_ln_bwd with (att) and without the attention term, accumulating in place."""
    c = _row_inputs(B, G, TV, K)
    d = _to(c, _dev())
    vp, wp = (c["vpart"], c["wp"]) if att else (None, None)
    fb = dict(out=Buf(B, G), out_bf=Buf(B, G, dt=BF16), xhat=Buf(B, G), rstd=Buf(B), vsum=Buf(B, G))
    _lib.call("pbx_row_ln_fwd", d["u"].data_ptr(), d["bias"].data_ptr(), d["res"].data_ptr(),
              d["vpart"].data_ptr() if att else None, TV if att else 0, d["wp"].data_ptr() if att else None,
              K if att else 0, d["nw"].data_ptr(), d["nb"].data_ptr(), fb["out"].full.data_ptr(),
              fb["out_bf"].full.data_ptr(), fb["xhat"].full.data_ptr(), fb["rstd"].full.data_ptr(),
              fb["vsum"].full.data_ptr() if att else None, B, G, EPS, _st())
    torch.cuda.synchronize()
    for n, buf in fb.items():
        if n == "vsum" and not att:
            assert buf.untouched(), "vsum written without vpart"
        else:
            buf.assert_written(n)
    k = _cpu(fb)
    o64, o32 = [go.row_ln_fwd(c["u"], c["bias"], c["res"], vp, wp, c["nw"], c["nb"], EPS, dt) for dt in (F64, F32)]
    # a GELU error e in z moves rstd by <= rstd^2 e, xhat by <= rstd (2 + |xhat|) e and out by |nw| times that
    rs, xm = float(o64["rstd"].max()), float(o64["xhat"].abs().max())
    mag = o64["_mag"]
    if att:
        go.check("row.vsum", k["vsum"], o64["vsum"], o32["vsum"], 0.0, LEDGER)
    go.check("row.rstd", k["rstd"], o64["rstd"], o32["rstd"], mag * rs * rs, LEDGER)
    go.check("row.xhat", k["xhat"], o64["xhat"], o32["xhat"], mag * rs * (2 + xm), LEDGER)
    go.check("row.out", k["out"], o64["out"], o32["out"], mag * rs * (2 + xm) * float(c["nw"].abs().max()), LEDGER)
    assert torch.equal(k["out_bf"], go.rne_bf16(k["out"])), "out_bf is not the RNE bf16 of the stored out"

    gen = torch.Generator().manual_seed(13)
    pre = dict(dgamma=torch.randn(G, generator=gen), dbeta=torch.randn(G, generator=gen),
               dbias=torch.randn(G, generator=gen), dwp=torch.randn(K, generator=gen) if att else None)
    bb = dict(du=Buf(B, G, dt=BF16), dres=Buf(B, G), dvs=Buf(B, G))
    acc = {n: (None if v is None else Buf(v.numel(), fill=v)) for n, v in pre.items()}
    p = lambda t: None if t is None else t.full.data_ptr()  # noqa: E731
    _lib.call("pbx_row_ln_bwd", d["dout"].data_ptr(), fb["xhat"].full.data_ptr(), fb["rstd"].full.data_ptr(),
              d["nw"].data_ptr(), d["u"].data_ptr(), d["bias"].data_ptr(), p(acc["dgamma"]), p(acc["dbeta"]),
              p(acc["dbias"]), p(bb["du"]), p(bb["dres"]), fb["vsum"].full.data_ptr() if att else None,
              d["wp"].data_ptr() if att else None, K if att else 0, p(acc["dwp"]), p(bb["dvs"]) if att else None,
              B, G, _st())
    torch.cuda.synchronize()
    for n, buf in {**bb, **acc}.items():
        if buf is None:
            continue
        if n == "dvs" and not att:
            assert buf.untouched()
        else:
            buf.assert_written(n)
    got = _cpu({**bb, **acc})
    r64, r32 = [go.row_ln_bwd(c["dout"], k["xhat"], k["rstd"], c["nw"], c["u"], c["bias"], k["vsum"] if att else None,
                              wp, dt) for dt in (F64, F32)]
    go.check_bf16("row.du", got["du"], r64["du"], r32["du"], r64["_mag_du"], LEDGER)
    go.check("row.dres", got["dres"], r64["dres"], r32["dres"], 0.0, LEDGER)
    for n in ("dgamma", "dbeta", "dbias") + (("dwp",) if att else ()):
        go.check("row." + n, got[n], r64[n] + pre[n].to(F64), r32[n] + pre[n],
                 r64["_mag_dbias"] if n == "dbias" else 0.0, LEDGER)
    if att:
        go.check("row.dvs", got["dvs"], r64["dvs"], r32["dvs"], 0.0, LEDGER)


@pytest.mark.parametrize("M,N", [(37, 130), (300, 130), (256, 512)])
def test_bias_gelu_kernels(M, N):
    """pbx_bias_gelu and pbx_bias_gelu_bwd, atomic and slab form (M = 300: two rows a block, empty blocks)."""
    gen = torch.Generator().manual_seed(M + N)
    u, bias, dout = torch.randn(M, N, generator=gen), torch.randn(N, generator=gen) * 0.1, torch.randn(M, N, generator=gen)
    pre = torch.randn(N, generator=gen)
    ud, bd, dd = u.to(_dev()), bias.to(_dev()), dout.to(_dev())
    out, out_bf = Buf(M, N), Buf(M, N, dt=BF16)
    _lib.call("pbx_bias_gelu", ud.data_ptr(), bd.data_ptr(), out.full.data_ptr(), out_bf.full.data_ptr(), M, N, _st())
    torch.cuda.synchronize()
    out.assert_written("out")
    out_bf.assert_written("out_bf")
    go.check("bg.out", out.v.cpu(), go.bias_gelu(u, bias, F64), go.bias_gelu(u, bias, F32),
             float((u + bias).abs().max()), LEDGER)
    assert torch.equal(out_bf.v.cpu(), go.rne_bf16(out.v.cpu()))
    o64, o32 = go.bias_gelu_bwd(dout, u, bias, F64), go.bias_gelu_bwd(dout, u, bias, F32)
    res = {}
    for form in ("atomic", "slab", "slab2"):
        du, db = Buf(M, N, dt=BF16), Buf(N, fill=pre)
        sl = None if form == "atomic" else torch.full((min(M, gt.BGB_ROWS), N), float("nan"), dtype=F32, device=_dev())
        _lib.call("pbx_bias_gelu_bwd", dd.data_ptr(), ud.data_ptr(), bd.data_ptr(), du.full.data_ptr(),
                  db.full.data_ptr(), M, N, _lib.ptr(sl), _st())
        torch.cuda.synchronize()
        du.assert_written("du")
        db.assert_written("dbias")
        res[form] = (du.v.cpu(), db.v.cpu())
        if form != "slab2":
            go.check_bf16("bg.du", res[form][0], o64["du"], o32["du"], o64["_mag_du"], LEDGER)
            go.check("bg.dbias", res[form][1], o64["dbias"] + pre.to(F64), o32["dbias"] + pre, o64["_mag_dbias"], LEDGER)
    assert torch.equal(res["slab"][1], res["slab2"][1]) and torch.equal(res["slab"][0].float(), res["slab2"][0].float())
    assert torch.equal(res["slab"][0].float(), res["atomic"][0].float())


# ---- through autograd -----------------------------------------------------------------------------------
ORDER = ["w1", "b1", "n1w", "n1b", "w2", "b2", "n2w", "n2b"]


def _apply(fn, inp_d, par_d, dg2_d, dgb_d, NGL, packed=None):
    leaves = {n: par_d[n].clone().requires_grad_() for n in ORDER}
    leaves["wp"] = inp_d["wp"].clone().requires_grad_()
    for n in ("wgl", "bgl"):
        leaves[n] = par_d[n].clone().requires_grad_() if NGL else None
    g = inp_d["g"].clone().requires_grad_()
    vp = inp_d["vpart"].clone().requires_grad_()
    args = [g, inp_d["g_bf"], vp] + [leaves[n] for n in ORDER + ["wp", "wgl", "bgl"]]
    g2, g2_bf, gb = fn.apply(*args, packed) if packed is not None else fn.apply(*args)
    loss = (g2 * dg2_d).sum() + ((gb * dgb_d).sum() if NGL else 0.0)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (None if t is None else t.grad.detach().cpu()) for n, t in leaves.items()}
    grads["g"], grads["vpart"] = g.grad.detach().cpu(), vp.grad.detach().cpu()
    return dict(g2=g2.detach().cpu(), g2_bf=g2_bf.detach().cpu(), gb=gb.detach().cpu()), grads


@pytest.mark.parametrize("TV,det", [(8, False), (17, False), (8, True)])
def test_fused_block_through_autograd(TV, det):
    """FusedGlobalBlockFn at (37, 512, 128): outputs and dg bitwise equal to the direct launches on the same
    inputs, dvpart [B, TV, G] with every slice the oracle's dvs, the weight gradients against fp64 products of
    the stored operands, the column-sum gradients against the oracle (``det``: in deterministic mode, the slab
    form), and ``packed=`` from pack_batch bitwise equal to the pack_glob path.  TV = 17 takes the pre-summed
    path (TV > 16)."""
    B, G, NGL, K = 37, 512, 128, 64
    (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d) = _fwd_case(B, G, NGL, TV, K, seed=9)
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        if det:
            determinism.enable()
            assert determinism.fused_deterministic()
        outs, grads = _apply(gt.FusedGlobalBlockFn, inp_d, par_d, dg2_d, dgb_d, NGL)
        imgs = [torch.empty(n * G, dtype=BF16, device=_dev()) for n in (G, G, G, G, NGL, NGL)]
        gt.pack_batch([(1, par_d["w1"], imgs[0], imgs[1], G, G), (1, par_d["w2"], imgs[2], imgs[3], G, G),
                       (1, par_d["wgl"], imgs[4], imgs[5], NGL, G)])
        outs_p, grads_p = _apply(gt.FusedGlobalBlockFn, inp_d, par_d, dg2_d, dgb_d, NGL, packed=tuple(imgs))
    finally:
        if det:
            torch.use_deterministic_algorithms(prev)
            determinism._STATE["on"] = False
    for n in outs:
        assert torch.equal(outs[n].float(), outs_p[n].float()), f"{n}: packed= differs from the pack_glob path"
    assert torch.equal(grads["g"], grads_p["g"])
    # the direct launches on the same inputs (TV > 16: the partials pre-summed, as the op does)
    pk = _packs(par_d)
    d_in = dict(inp_d)
    TVk = TV
    if TV > 16:
        d_in["vpart"], TVk = inp_d["vpart"].sum(dim=1, keepdim=True), 1
    fb = launch_fwd(d_in, par_d, pk, B, G, NGL, TVk, K)
    k = _cpu(fb)
    k["g_bf"] = inp["g_bf"]
    for n in ("g2", "g2_bf", "gb"):
        assert torch.equal(outs[n].float(), k[n].float()), f"{n}: op output differs from the direct launch"
    go.check("vsum|TV", k["vsum"], go.st_vsum(inp["vpart"], F64), go.st_vsum(inp["vpart"], F32), 0.0, LEDGER)
    kd = {n: (None if v is None else v.v) for n, v in fb.items()}
    zero = {n: torch.zeros(s) for n, s in [("db1", G), ("dn1w", G), ("dn1b", G), ("db2", G), ("dn2w", G),
                                           ("dn2b", G), ("dbgl", NGL), ("dwp", K)]}
    bb = _cpu(launch_bwd(dg2_d, dgb_d, kd, par_d, inp_d["wp"], pk, B, G, NGL, K, det, zero))
    assert torch.equal(grads["g"], bb["dg"]), "dg: op gradient differs from the direct launch"
    bk = {n: bb[n] for n in ("dugl", "du2", "du1")}
    o64 = go.backward_stages(dg2, dgb, k, par, inp["wp"], bk, F64)
    o32 = go.backward_stages(dg2, dgb, k, par, inp["wp"], bk, F32)
    assert grads["vpart"].shape == (B, TV, G)
    for t in range(TV):
        go.check("dvpart[t]", grads["vpart"][:, t], o64["dvs"], o32["dvs"], 0.0, LEDGER if t == 0 else None)
    for n, w in (("dW1", "w1"), ("dW2", "w2"), ("dWgl", "wgl")):
        go.check(n, grads[w], o64[n], o32[n], 0.0, LEDGER)
    tag = "|det" if det else "|op"
    for n, p in (("db1", "b1"), ("dn1w", "n1w"), ("dn1b", "n1b"), ("db2", "b2"), ("dn2w", "n2w"), ("dn2b", "n2b"),
                 ("dbgl", "bgl"), ("dwp", "wp")):
        go.check(n + tag, grads[p], o64[n], o32[n], o64.get("_mag_" + n, 0.0), LEDGER)
        if det:
            assert torch.equal(grads[p], grads_p[p]), f"{n}: deterministic mode, two runs differ"


def test_general_block_through_autograd():
    """GlobalBlockFn at (24, 384, 128): outputs and dg bitwise equal to the same launcher sequence called
    directly, every stage of it against the oracle with u given, dvpart slices against the oracle's dvs."""
    B, G, NGL, TV, K = 24, 384, 128, 2, 64
    (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d) = _fwd_case(B, G, NGL, TV, K, seed=7)
    outs, grads = _apply(gt.GlobalBlockFn, inp_d, par_d, dg2_d, dgb_d, NGL)
    e = lambda *s, dt=F32: torch.empty(s, dtype=dt, device=_dev())  # noqa: E731
    st = _st()
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def ln_fwd(u, b, res, vp, wp, nw, nb):
        o = dict(out=e(B, G), out_bf=e(B, G, dt=BF16), xhat=e(B, G), rstd=e(B), vsum=e(B, G) if vp is not None else None)
        _lib.call("pbx_row_ln_fwd", P(u), P(b), P(res), P(vp), TV if vp is not None else 0, P(wp),
                  K if vp is not None else 0, P(nw), P(nb), P(o["out"]), P(o["out_bf"]), P(o["xhat"]), P(o["rstd"]),
                  P(o["vsum"]), B, G, EPS, st)
        return o

    u1 = gt.mm32(inp_d["g_bf"], gt.bf16_of(par_d["w1"]).t())
    s1 = ln_fwd(u1, par_d["b1"], inp_d["g"], inp_d["vpart"], inp_d["wp"], par_d["n1w"], par_d["n1b"])
    u2 = gt.mm32(s1["out_bf"], gt.bf16_of(par_d["w2"]).t())
    s2 = ln_fwd(u2, par_d["b2"], s1["out"], None, None, par_d["n2w"], par_d["n2b"])
    ugl = gt.mm32(s2["out_bf"], gt.bf16_of(par_d["wgl"]).t())
    gb = torch.empty_like(ugl)
    _lib.call("pbx_bias_gelu", P(ugl), P(par_d["bgl"]), P(gb), None, B, NGL, st)
    torch.cuda.synchronize()
    assert torch.equal(outs["g2"], s2["out"].cpu()) and torch.equal(outs["gb"], gb.cpu())
    assert torch.equal(outs["g2_bf"].float(), s2["out_bf"].cpu().float())
    for tag, u, b, res, vp, wp, nw, nb, s in (("gen1", u1, "b1", inp["g"], inp["vpart"], inp["wp"], "n1w", "n1b", s1),
                                               ("gen2", u2, "b2", s1["out"].cpu(), None, None, "n2w", "n2b", s2)):
        o64, o32 = [go.row_ln_fwd(u.cpu(), par[b], res, vp, wp, par[nw], par[nb], EPS, dt) for dt in (F64, F32)]
        rs, xm, mag = float(o64["rstd"].max()), float(o64["xhat"].abs().max()), o64["_mag"]
        go.check(tag + ".xhat", s["xhat"].cpu(), o64["xhat"], o32["xhat"], mag * rs * (2 + xm), LEDGER)
        go.check(tag + ".out", s["out"].cpu(), o64["out"], o32["out"],
                 mag * rs * (2 + xm) * float(par[nw].abs().max()), LEDGER)
    # the products themselves: the in-tree GEMM against fp64 from the same bf16 operands
    for tag, u, x, w in (("gen.u1", u1, inp["g_bf"], "w1"), ("gen.u2", u2, s1["out_bf"].cpu(), "w2"),
                         ("gen.ugl", ugl, s2["out_bf"].cpu(), "wgl")):
        zero = torch.zeros(par[w].shape[0])
        go.check(tag, u.cpu(), go.st_pre(x, par[w], zero, F64), go.st_pre(x, par[w], zero, F32), 0.0, LEDGER)
    # backward, the same launcher sequence as the op
    dugl = e(B, NGL, dt=BF16)
    dbgl = torch.zeros(NGL, device=_dev())
    _lib.call("pbx_bias_gelu_bwd", P(dgb_d), P(ugl), P(par_d["bgl"]), P(dugl), P(dbgl), B, NGL, None, st)
    dy2 = gt.addmm_new(dg2_d, dugl, gt.bf16_of(par_d["wgl"]))
    z = lambda n: torch.zeros(n, device=_dev())  # noqa: E731
    du2, dg1 = e(B, G, dt=BF16), e(B, G)
    acc2 = [z(G), z(G), z(G)]
    _lib.call("pbx_row_ln_bwd", P(dy2), P(s2["xhat"]), P(s2["rstd"]), P(par_d["n2w"]), P(u2), P(par_d["b2"]),
              P(acc2[0]), P(acc2[1]), P(acc2[2]), P(du2), P(dg1), None, None, 0, None, None, B, G, st)
    ds2 = dg1.clone()
    gt.addmm_into(dg1, du2, gt.bf16_of(par_d["w2"]))
    du1, dg, dvs, dwp = e(B, G, dt=BF16), e(B, G), e(B, G), z(K)
    acc1 = [z(G), z(G), z(G)]
    _lib.call("pbx_row_ln_bwd", P(dg1), P(s1["xhat"]), P(s1["rstd"]), P(par_d["n1w"]), P(u1), P(par_d["b1"]),
              P(acc1[0]), P(acc1[1]), P(acc1[2]), P(du1), P(dg), P(s1["vsum"]), P(inp_d["wp"]), K, P(dwp), P(dvs),
              B, G, st)
    gt.addmm_into(dg, du1, gt.bf16_of(par_d["w1"]))
    torch.cuda.synchronize()
    assert torch.equal(grads["g"], dg.cpu()), "dg: op gradient differs from the direct launches"
    r64, r32 = [go.row_ln_bwd(dg1.cpu(), s1["xhat"].cpu(), s1["rstd"].cpu(), par["n1w"], u1.cpu(), par["b1"],
                              s1["vsum"].cpu(), inp["wp"], dt) for dt in (F64, F32)]
    assert grads["vpart"].shape == (B, TV, G)
    for t in range(TV):
        go.check("gen.dvpart[t]", grads["vpart"][:, t], r64["dvs"], r32["dvs"], 0.0, LEDGER if t == 0 else None)
    go.check("gen.dwp", grads["wp"], r64["dwp"], r32["dwp"], 0.0, LEDGER)
    go.check("gen.db1", grads["b1"], r64["dbias"], r32["dbias"], r64["_mag_dbias"], LEDGER)
    go.check("gen.dn1w", grads["n1w"], r64["dgamma"], r32["dgamma"], 0.0, LEDGER)
    q64, q32 = [go.row_ln_bwd(dy2.cpu(), s2["xhat"].cpu(), s2["rstd"].cpu(), par["n2w"], u2.cpu(), par["b2"], None,
                              None, dt) for dt in (F64, F32)]
    go.check("gen.ds2", ds2.cpu(), q64["dres"], q32["dres"], 0.0, LEDGER)
    go.check("gen.db2", grads["b2"], q64["dbias"], q32["dbias"], q64["_mag_dbias"], LEDGER)
    for n, a, x in (("gen.dW1", du1, inp["g_bf"]), ("gen.dW2", du2, s1["out_bf"].cpu()), ("gen.dWgl", dugl, s2["out_bf"].cpu())):
        w = {"gen.dW1": "w1", "gen.dW2": "w2", "gen.dWgl": "wgl"}[n]
        go.check(n, grads[w], a.cpu().to(F64).t() @ x.to(F64), a.cpu().float().t() @ x.float(), 0.0, LEDGER)


# ---- invalid arguments ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,over", [("fwd", dict(G=384)), ("fwd", dict(NGL=64)), ("fwd", dict(B=0)),
                                        ("bwd", dict(G=384)), ("bwd", dict(NGL=64)), ("bwd", dict(B=0)),
                                        ("bwd", dict(K=513))])
def test_fused_launchers_reject_invalid(which, over):
    """Unsupported shapes raise and leave the sentinel-filled outputs untouched."""
    B, G, NGL, TV, K = 16, 256, 128, 2, 64
    (inp, par, dg2, dgb), (inp_d, par_d, dg2_d, dgb_d) = _fwd_case(B, G, NGL, TV, K)
    pk = _packs(par_d)
    a = dict(B=B, G=G, NGL=NGL, K=K)
    a.update(over)
    if which == "fwd":
        bufs = launch_fwd(inp_d, par_d, pk, B, G, NGL, TV, K)
        for buf in bufs.values():
            buf._sentinel(buf.full)
        with pytest.raises(_lib.HipError):
            launch_fwd(inp_d, par_d, pk, a["B"], a["G"], a["NGL"], TV, a["K"], bufs=bufs)
    else:
        fb = launch_fwd(inp_d, par_d, pk, B, G, NGL, TV, K)
        kd = {n: v.v for n, v in fb.items()}
        pre = {n: torch.zeros(s) for n, s in [("db1", G), ("dn1w", G), ("dn1b", G), ("db2", G), ("dn2w", G),
                                              ("dn2b", G), ("dbgl", NGL), ("dwp", 600)]}
        bufs = launch_bwd(dg2_d, dgb_d, kd, par_d, inp_d["wp"], pk, B, G, NGL, K, False, pre)
        for buf in bufs.values():
            buf._sentinel(buf.full)
        with pytest.raises(_lib.HipError):
            launch_bwd(dg2_d, dgb_d, kd, par_d, inp_d["wp"], pk, a["B"], a["G"], a["NGL"], a["K"], True, pre,
                       bufs=bufs, slab_rows=1)
    torch.cuda.synchronize()
    for n, buf in bufs.items():
        assert buf.untouched(), f"{n}: written by a rejected launch"


@pytest.mark.parametrize("which", ["fwd_G1025", "bwd_G1025", "bwd_K257"])
def test_row_launchers_reject_invalid(which):
    B, G, K = 2, 1025, 257
    d = _to(_row_inputs(B, G, 1, K), _dev())
    bufs = dict(out=Buf(B, G), out_bf=Buf(B, G, dt=BF16), xhat=Buf(B, G), rstd=Buf(B), vsum=Buf(B, G),
                du=Buf(B, G, dt=BF16), dres=Buf(B, G), dvs=Buf(B, G), acc=Buf(3, G), dwp=Buf(K))
    P = lambda n: bufs[n].full.data_ptr()  # noqa: E731
    xh, rs = torch.randn(B, G, device=_dev()), torch.ones(B, device=_dev())
    with pytest.raises(_lib.HipError):
        if which == "fwd_G1025":
            _lib.call("pbx_row_ln_fwd", d["u"].data_ptr(), d["bias"].data_ptr(), d["res"].data_ptr(),
                      d["vpart"].data_ptr(), 1, d["wp"].data_ptr(), K, d["nw"].data_ptr(), d["nb"].data_ptr(),
                      P("out"), P("out_bf"), P("xhat"), P("rstd"), P("vsum"), B, G, EPS, _st())
        else:
            Gb = G if which == "bwd_G1025" else 1024
            Kb = 48 if which == "bwd_G1025" else K
            acc = bufs["acc"].full
            _lib.call("pbx_row_ln_bwd", d["dout"].data_ptr(), xh.data_ptr(), rs.data_ptr(), d["nw"].data_ptr(),
                      d["u"].data_ptr(), d["bias"].data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(),
                      acc[2].data_ptr(), P("du"), P("dres"), d["res"].data_ptr(), d["wp"].data_ptr(), Kb, P("dwp"),
                      P("dvs"), B, Gb, _st())
    torch.cuda.synchronize()
    for n, buf in bufs.items():
        assert buf.untouched(), f"{n}: written by a rejected launch"
