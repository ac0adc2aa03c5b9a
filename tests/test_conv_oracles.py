"""CPU: the conv oracles of tests/conv_oracles.py are right on their own, so the GPU assertions of
tests/test_hip_conv_exact.py mean something.

* With every rounding switched off, the chained fp64 stages (forward, LayerNorm-1 finalize, data gradient) agree
  with fp64 ``torch.autograd`` of the plain block expression (the conv / GELU / residual part of ``torch_local`` in
  tests/test_hip_local_track.py and its LayerNorm-1) to 1e-12 relative.
* With the roundings on, an fp32 stand-in kernel (taps summed in the other order) passes every check.
* Nine altered stand-ins (``conv_oracles.MUTANTS``): eight are rejected on the tensors listed in ``REJECTS``, one
  (an FMA contraction) must be accepted.
* The claim of ``ops/csrc/common.h`` for the fitted GELU core is checked on a dense fp64 grid, and the ambiguous
  shares of the hidden roundings stay under the 10 % condition."""
import pytest
import torch
import torch.nn.functional as F

import conv_oracles as co
from conv_oracles import BM, C, DIL, EPS, F32, F64

ROWS = ("rows", BM)


def test_fitted_gelu_claim():
    """common.h: the fitted logistic core is within 2.9e-4 of the erf GELU and 7.8e-4 of its derivative on
    [-14, 14] (figures given to two digits: the assertion is 'rounds to no more than the stated figure')."""
    x = co.grid64()
    (gf, df), (ge, de) = co.gelu_pair(x, "fitted"), co.gelu_pair(x, "exact")
    eg, ed = float((gf - ge).abs().max()), float((df - de).abs().max())
    print(f"fitted GELU: max |err| {eg:.4e} (claimed {co.FIT_CLAIM[0]}), GELU' {ed:.4e} (claimed {co.FIT_CLAIM[1]})")
    assert torch.allclose(ge, F.gelu(x), rtol=0, atol=1e-14)
    assert eg < co.FIT_CLAIM[0] + 0.05e-4 and ed < co.FIT_CLAIM[1] + 0.05e-4
    for mode in ("fitted", "exact"):                       # the Lipschitz constants the intervals are scaled by
        lg, lgd = co.lipschitz(mode)
        print(f"{mode}: Lip(GELU) {lg:.4f}  Lip(GELU') {lgd:.4f}")
        assert 1.0 < lg < 1.2 and 0.7 < lgd < 1.0


def _as64(c):
    return {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}


@pytest.mark.parametrize("B,L,bm1,ts1", [(2, 36, BM, 18), (3, 130, BM, 65), (2, 257, 2, 600)])
def test_oracle_agrees_with_fp64_autograd(B, L, bm1, ts1):
    """Rounding off, erf GELU: s1, dS1, dgb, both dpre and dx against fp64 autograd; the LayerNorm statistics go
    through the (mean, M2) partials of ``bm1`` rows and the backward constants through ``ts1`` partial sums."""
    c = _as64(co.make_case(B, L))
    k = co.play_forward(c, "exact", ("rows", bm1), dt=F64, rounding=False)
    k["st1"] = k["stats"]
    k["sums1"] = co.make_sums1(c["dh1"], k["s1"], c["g1"], k["st1"], bm1, L, ts1, out_dt=F64)
    got = co.play_backward(c, k, bm1, fused=False, dt=F64, rounding=False)

    x, gb = c["x"].clone().requires_grad_(), c["gb"].clone().requires_grad_()
    xt = x.transpose(1, 2)
    pn = F.conv1d(xt, c["wn"], c["bn"], padding="same", dilation=1).transpose(1, 2)
    pw = F.conv1d(xt, c["ww"], c["bw"], padding="same", dilation=DIL).transpose(1, 2)
    s1 = x + F.gelu(pn) + F.gelu(pw) + gb.unsqueeze(1)
    s1.retain_grad()
    h1 = F.layer_norm(s1, (L, C), c["g1"], torch.zeros(L, C, dtype=F64), eps=EPS)
    dx, dgb, ds1, dpn, dpw = torch.autograd.grad((h1 * c["dh1"]).sum(), [x, gb, s1, pn, pw])
    pairs = [("s1", k["s1"], s1.detach()), ("ds1", got["ds1"], ds1), ("dgb", got["dgb"] - c["dgb0"], dgb),
             ("dpn", got["dpn"], dpn), ("dpw", got["dpw"], dpw), ("dx", got["dx"], dx)]
    for n, a, b in pairs:
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        print(f"{n:4s} err {err:.3e}  ref {ref:.3e}")
        assert a.shape == b.shape and err <= 1e-12 * ref, (n, err, ref)


def _played(c, mode, layout=ROWS, bm1=BM, ts1=None, mutant=None, fused=False):
    """The stand-in's forward, then its backward from the forward's own outputs (as the GPU test chains them)."""
    L = c["L"]
    k = co.play_forward(c, mode, layout, mutant=mutant)
    kb = dict(k)
    if layout == ROWS and bm1 != BM:                       # synthetic partial tables
        m, M2, _ = co.st_stats(k["s1"], L, ("rows", bm1), F64)
        kb["st1"] = torch.stack([m, M2], dim=-1).to(F32)
    else:
        kb["st1"] = k["stats"]
    kb["sums1"] = co.make_sums1(c["dh1"], k["s1"], c["g1"], kb["st1"], bm1, L, ts1 or (L + 1) // 2)
    return k, kb, co.play_backward(c, kb, bm1, fused, mutant=mutant)


def _check_all(c, mode, k, kb, got, bm1, fused, fails=None, led=None, layout=ROWS):
    co.check_forward(c, k, mode, layout, led, fails)
    if fused:
        co.check_dgrad_fin(c, kb, bm1, got, EPS, led, fails)
    else:
        co.check_ln1(c, kb, got, bm1, EPS, led, fails)
        cc = dict(c, ds1=got["ds1"])
        co.check_dgrad(cc, kb["gdn"], kb["gdw"], got, led, fails)


@pytest.mark.parametrize("mode", ["fitted", "exact"])
@pytest.mark.parametrize("B,L", [(2, 36), (3, 130), (2, 257), (2, 300)])
def test_standin_passes_every_check(B, L, mode):
    """The stand-in alone is inside every condition: forward, ln1_finalize + conv_dgrad4x, conv_dgrad4f, the halo
    forms, the token layout of the partials and the synthetic (BM1 = 2, TS1 = 600) tables.  The ambiguous shares
    are re-measured: (2, 300) gave 2.3 % for both pre-activations, (2, 257) 2.3 % for dS1."""
    led = co.ConvLedger()
    c = co.make_case(B, L, gb_shift=3.0 if L == 130 else 0.0)
    for fused in (False, True):
        k, kb, got = _played(c, mode, fused=fused)
        _check_all(c, mode, k, kb, got, BM, fused, None, led)
    k, kb, got = _played(c, mode, bm1=2, ts1=600, fused=True)
    co.check_dgrad_fin(c, kb, 2, got, EPS, led, None, tag="dgrad4f|synthetic")
    ch = co.make_case(B, L, lo=20, hi=20)                  # halo rows: forward and the plain data gradient
    kh = co.play_forward(ch, mode, ROWS)
    co.check_forward(ch, kh, mode, ROWS, led, None, tag="fwd|halo")
    co.check_dgrad(ch, ch["gdn"], ch["gdw"], co.play_backward(ch, None, BM, False, ch["gdn"], ch["gdw"], ch["ds1"]),
                   led, None, tag="dgrad4x|halo")
    shares = {n: v for n, v in led.notes.items() if n.startswith("ambiguous")}
    assert len(shares) >= 6 and max(shares.values()) < co.AMBIGUOUS_MAX, shares
    if (B, L) == (2, 300):
        assert 0.01 < shares["ambiguous fwd.pre_n"] < 0.05 and 0.01 < shares["ambiguous fwd.pre_w"] < 0.05, shares
    if (B, L) == (2, 257):
        assert 0.01 < shares["ambiguous dgrad4f.ds1"] < 0.05, shares


def test_standin_token_layout():
    """The partials of conv_fwd_tok ([tile][half][wave], 8 positions x 64 channels) and pbx_embed_dpre."""
    c = co.make_case(2, 256, tok=True)
    lay = ("tok",)
    k = co.play_forward(c, "fitted", lay)
    assert k["stats"].shape == (2, 64, 2)
    co.check_forward(c, k, "fitted", lay)
    # the (T1, BM1) = (L / 4, 4) reading of these partials gives the statistics of the whole sample
    mean, rstd, _, _ = co.st_ln1_consts(k["stats"], 4, torch.zeros(2, 1, 2), 256, EPS, F64)
    s = k["s1"].to(F64).reshape(2, -1)
    assert torch.allclose(mean, s.mean(1), rtol=0, atol=1e-5) and torch.allclose(rstd, torch.rsqrt(s.var(1, unbiased=False) + EPS), rtol=1e-5)
    ds1 = c["ds1"]
    dpn, dpw = co.rne_bf16(ds1.float() * k["gdn"].float()), co.rne_bf16(ds1.float() * k["gdw"].float())
    dE = c["dE0"].index_add(0, c["tok"].reshape(-1), ds1.float().reshape(-1, C))
    co.check_embed_dpre(c, ds1, k["gdn"], k["gdw"], dict(dpn=dpn, dpw=dpw, dE=dE))
    fails = []
    co.check_embed_dpre(c, ds1, k["gdn"], k["gdw"], dict(dpn=dpn, dpw=co.trunc_bf16(ds1.float() * k["gdw"].float()),
                                                          dE=dE + 1e-3), None, fails)
    assert {n for n, _ in fails} == {"embed_dpre.dpw", "embed_dpre.dE"}


# mutant -> (case, the tensors that must reject it; others may as well).  fma_contracted_sum: see below.
REJECTS = {
    "drop_edge_tap": (dict(B=2, L=300), {"fwd.gdw(bf16)", "fwd.s1(bf16)"}),
    "clamp_pad": (dict(B=2, L=300), {"fwd.gdn(bf16)", "fwd.gdw(bf16)", "fwd.s1(bf16)"}),
    "bf16_truncate": (dict(B=2, L=300), {"fwd.gdn(bf16)", "fwd.gdw(bf16)", "fwd.s1(bf16)", "dgrad4x.dx(bf16)",
                                         "dgrad4x.dpn", "dgrad4x.dpw", "ln1.ds1"}),
    "pre_not_rounded": (dict(B=2, L=300), {"fwd.gdn(bf16)", "fwd.gdw(bf16)", "fwd.s1(bf16)"}),
    "halo_off_by_one": (dict(B=2, L=300, lo=20, hi=20), {"fwd.gdn(bf16)", "fwd.gdw(bf16)", "fwd.s1(bf16)"}),
    "dgrad_shift_sign": (dict(B=2, L=300), {"dgrad4x.dx(bf16)"}),
    "chan_count_full_tile": (dict(B=3, L=130), {"ln1.ds1"}),
    "m2_dropped": (dict(B=3, L=130), {"ln1.ds1"}),
}


@pytest.mark.parametrize("mutant", sorted(REJECTS))
def test_mutant_is_rejected(mutant):
    """Each altered stand-in fails at least the listed tensors, and the healthy one fails none."""
    assert mutant in co.MUTANTS
    kw, want = REJECTS[mutant]
    c = co.make_case(**kw)
    halo = kw.get("lo", 0) > 0
    res = {}
    for mu in (None, mutant):
        fails = []
        if halo:
            co.check_forward(c, co.play_forward(c, "fitted", ROWS, mutant=mu), "fitted", ROWS, None, fails)
        else:
            k0, kb0, _ = _played(c, "fitted")              # the backward mutant runs on a healthy forward
            k, _, _ = _played(c, "fitted", mutant=mu)
            got = co.play_backward(c, kb0, BM, False, mutant=mu)
            co.check_forward(c, k, "fitted", ROWS, None, fails)
            co.check_ln1(c, kb0, got, BM, EPS, None, fails)
            co.check_dgrad(dict(c, ds1=got["ds1"]), kb0["gdn"], kb0["gdw"], got, None, fails)
        res[mu] = {n: m for n, m in fails}
    for n, m in res[mutant].items():
        print(f"{mutant}: {n}: {m}")
    assert not res[None], res[None]
    assert want <= set(res[mutant]), (mutant, sorted(res[mutant]))


def test_fma_contraction_is_accepted():
    """``x + G(pre_n)`` formed as one fma differs from the kernels' two roundings by an fp32 ulp of some elements:
    that is fp32 arithmetic, so the tolerance checks MUST accept it.  Only the bitwise conv_fwd5 = conv_fwd3
    test (tests/test_hip_conv_fwd5.py) tells the two apart -- do not tighten this oracle into a bit-match."""
    assert "fma_contracted_sum" in co.MUTANTS
    c = co.make_case(2, 300)
    k0, k = co.play_forward(c, "fitted", ROWS), co.play_forward(c, "fitted", ROWS, mutant="fma_contracted_sum")
    diff = int((k0["s1"].view(torch.int16) != k["s1"].view(torch.int16)).sum())
    print(f"fma_contracted_sum: {diff} of {k['s1'].numel()} s1 elements differ bitwise")
    assert diff > 0
    fails = []
    co.check_forward(c, k, "fitted", ROWS, None, fails)
    assert not fails, fails


def test_m2_term_is_exercised():
    """gb + 3: the one-pass M2 of the kernels errs by a few 2^-24 sumsq, far above a two-pass fp32 evaluation, and
    passes only through the 2^-24 sumsq term of the tolerance (the figures the issue measured: 1.3 .. 3.5)."""
    c = co.make_case(3, 130, gb_shift=3.0)
    led = co.ConvLedger()
    co.check_forward(c, co.play_forward(c, "fitted", ROWS), "fitted", ROWS, led)
    print(led.notes)
    assert led.notes["fwd.M2 err / two-pass e32"] > led.notes["fwd.M2 err / (2^-24 sumsq)"]
    assert led.notes["fwd.M2 err / (2^-24 sumsq)"] < co.MARGIN
