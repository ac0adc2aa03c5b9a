"""CPU: the oracles of tests/ln_oracles.py are right on their own, so the GPU assertions of
tests/test_hip_ln_exact.py mean something.

* With every rounding switched off, the chained fp64 stages agree with fp64 ``torch.autograd`` of the plain
  expression (``F.layer_norm`` over (L, C), a linear layer, erf GELU, the residual, a second LayerNorm) to 1e-12
  relative, in every backward output.
* With the roundings on, an fp32 stand-in kernel passes every check in both GELU modes.
* Twelve altered stand-ins (``ln_oracles.MUTANTS``) are each rejected on the tensors listed in ``REJECTS``.
* The conditions on the ambiguous shares and the drifts hold on every case of the GPU file (built here by
  ``make_case`` with the same arguments), from the reference alone.
* With the inputs of tests/test_hip_ln_inflight.py three of the mutants stay under that file's bounds: why the
  inputs here differ.
* A constructed counter-example for the one place where the yardstick is floored (half an fp32 ulp)."""
import pytest
import torch
import torch.nn.functional as F

import ln_oracles as lo
from ln_oracles import C, EPS, F32, F64

# the cases of tests/test_hip_ln_exact.py; FWD_WALK_B is what {g, g D + 1, g (2 D + 1) - 1, g (2 D + 1)} gives at
# 256 CUs (g = 4) with the ring depth D = 1 of ln.hip (the GPU file takes both from the device and the library)
FWD_WALK_B = (4, 5, 11, 12)
FWD_CASES = [(B, L, 128) for L in (4096, 4090) for B in FWD_WALK_B] + [(1, 33, 128), (3, 64, 128), (4, 4096, 4),
                                                                       (4, 4090, 4)]
BWD_CASES = [(1, 512), (16, 512), (17, 512), (37, 512), (33, 511), (2, 33), (80, 64), (3, 514), (17, 515), (2, 1026)]


def _as64(c):
    return {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}


@pytest.mark.parametrize("B,L,bm1", [(2, 33, 128), (3, 70, 4), (2, 130, 32)])
def test_oracle_agrees_with_fp64_autograd(B, L, bm1):
    """Rounding off, erf GELU: s2, the constants, dh1, sums1 and the six gradients against fp64 autograd; the
    LayerNorm statistics go through (mean, M2) partials of ``bm1`` / 32 rows."""
    c = _as64(lo.make_case(B, L, bm1))
    c["st1"] = lo.tile_partials(c["s1"], bm1, L, F64)
    k = lo.play_forward(c, "exact", dt=F64, rounding=False)
    kb = dict(dh2=c["dh2"], s2=k["s2"], pre_l=k["pre_l"], st2=k["st2"], st1=c["st1"],
              sums2=lo.make_sums2(c["dh2"], k["s2"], c["g2"], L, out_dt=F64))
    got = lo.play_backward(c, kb, "exact", dt=F64, rounding=False)

    g1, be1, g2, wl, bl = (c[n].clone().requires_grad_() for n in ("g1", "be1", "g2", "wl", "bl"))
    be2 = torch.zeros(L, C, dtype=F64, requires_grad=True)
    h1 = F.layer_norm(c["s1"], (L, C), g1, be1, eps=EPS)
    h1.retain_grad()
    pre = h1 @ wl.t() + bl
    s2 = h1 + F.gelu(pre)
    h2 = F.layer_norm(s2, (L, C), g2, be2, eps=EPS)
    dg1, db1, dg2, db2, dwl, dbl, dh1 = torch.autograd.grad((h2 * c["dh2"]).sum(), [g1, be1, g2, be2, wl, bl, h1])
    xh1, xh2 = lo.plain_xhat(c["s1"]), lo.plain_xhat(s2.detach())
    dxh2, dxh1 = c["dh2"] * c["g2"], dh1 * c["g1"]
    flat = lambda t: t.reshape(B, -1)  # noqa: E731
    stats = lambda t: (flat(t).mean(1), torch.rsqrt(flat(t).var(1, unbiased=False) + EPS))  # noqa: E731
    consts = torch.stack([*stats(s2.detach()), flat(dxh2).mean(1), flat(dxh2 * xh2).mean(1), *stats(c["s1"])], dim=1)
    sums1 = torch.stack([lo._pair_sums(dxh1, L), lo._pair_sums(dxh1 * xh1, L)], dim=-1)
    pairs = [("s2", k["s2"], s2.detach()), ("pre", k["pre_l"], pre.detach()), ("dh1", got["dh1"], dh1),
             ("sums1.dxh", got["sums1"][..., 0], sums1[..., 0]), ("sums1.dxh_xhat", got["sums1"][..., 1], sums1[..., 1]),
             ("dg2", got["dg2"] - c["dg2_0"], dg2), ("db2", got["db2"] - c["db2_0"], db2),
             ("dg1", got["dg1"] - c["dg1_0"], dg1), ("db1", got["db1"] - c["db1_0"], db1),
             ("dwl", got["dwl"] - c["dwl_0"], dwl), ("dbl", got["dbl"] - c["dbl_0"], dbl)]
    pairs += [(f"consts.{n}", got["consts"][:, i], consts[:, i]) for i, n in enumerate(lo.CONSTS)]
    assert bool((got["consts"][:, 6:] == 0).all())
    for n, a, b in pairs:
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        print(f"{n:16s} err {err:.3e}  ref {ref:.3e}")
        assert a.shape == b.shape and err <= 1e-12 * max(ref, 1.0), (n, err, ref)
    # the preloads are of order 1 and the sums of order sqrt(B): subtracting them back costs an fp64 ulp of either,
    # which is what max(ref, 1) allows; every other pair is compared at its own scale


def _check_all(c, mode, k, got, fails=None, led=None):
    lo.check_forward(c, k, mode, led, fails)
    kb = lo.bwd_inputs(c)
    lo.check_consts(c, kb, got["consts"], led, fails)
    ref = lo.backward_ref(c, kb, got["consts"], mode, led, fails)
    lo.check_backward(c, got, ref, led, fails)
    return ref


STANDIN_CASES = [(2, 33, 128), (3, 70, 4), (5, 515, 128), (17, 130, 128), (1, 4090, 4)]


@pytest.mark.parametrize("mode", ["fitted", "exact"])
@pytest.mark.parametrize("B,L,bm1", STANDIN_CASES)
def test_standin_passes_every_check(B, L, bm1, mode):
    """The stand-in alone is inside every condition, and its hidden roundings lie in their admissible intervals.
    Its largest use of the 16 x margin is printed."""
    led = lo.ConvLedger()
    c = lo.make_case(B, L, bm1)
    k = lo.play_forward(c, mode)
    got = lo.play_backward(c, lo.bwd_inputs(c), mode)
    ref = _check_all(c, mode, k, got, None, led)
    lo.check_member("fwd.h1 (hidden)", k["hb"], *lo.forward_ref(c, mode)["h1"][:2])
    lo.check_member("bwd.dpre (hidden)", got["_dpre"], *ref["dpre"])
    lo.check_member("bwd.h1 (hidden)", got["_hv"], *ref["hv"])
    worst = max(led.worst.items(), key=lambda kv: kv[1])
    print(f"largest use of the margin: {worst[0]} at {worst[1]:.2f} of {lo.MARGIN:.0f}")
    assert worst[1] <= lo.MARGIN


# mutant -> (make_case arguments, gx, the tensors that must reject it; others may as well)
REJECTS = {
    "m2_term_dropped": ((3, 70, 128), None, {"bwd.dh1(bf16)", "bwd.dbl", "bwd.dwl"}),
    "m1_term_dropped": ((3, 70, 128), None, {"bwd.dh1(bf16)", "bwd.dbl", "bwd.dwl"}),
    "merge_no_between": ((2, 515, 128), None, {"fwd.pre_l(bf16)", "fwd.s2(bf16)", "bwd.consts.rstd1"}),
    "count_full_tile": ((2, 33, 128), None, {"fwd.mean", "fwd.M2"}),
    "bf16_truncate": ((3, 70, 128), None, {"fwd.pre_l(bf16)", "fwd.s2(bf16)", "bwd.dh1(bf16)"}),
    "residual_bf16": ((3, 70, 128), None, {"fwd.s2(bf16)"}),
    "gelu_on_rounded_pre": ((3, 70, 128), None, {"fwd.s2(bf16)"}),
    "chunk_tail_leaks": ((17, 33, 128), None, {"bwd.dg2", "bwd.db2"}),
    "odd_tail_row_live": ((2, 33, 128), None, {"bwd.sums1.dxh", "bwd.sums1.dxh_xhat"}),
    "dwl_reset_per_pair": ((2, 70, 128), 32, {"bwd.dwl"}),
    "sums1_from_unrounded_dh1": ((3, 70, 128), None, {"bwd.sums1.dxh", "bwd.sums1.dxh_xhat"}),
    "consts_slots_swapped": ((3, 70, 128), None, {"bwd.consts.m1", "bwd.consts.m2"}),
}


@pytest.mark.parametrize("mutant", lo.MUTANTS)
def test_mutant_is_rejected(mutant):
    """Each altered stand-in fails at least the listed tensors, and the healthy one fails none."""
    (B, L, bm1), gx, want = REJECTS[mutant]
    c = lo.make_case(B, L, bm1)
    res = {}
    for mu in (None, mutant):
        fails = []
        k = lo.play_forward(c, "fitted", mutant=mu)
        got = lo.play_backward(c, lo.bwd_inputs(c), "fitted", mutant=mu, gx=gx)
        _check_all(c, "fitted", k, got, fails)
        res[mu] = {n: m for n, m in fails}
    for n, m in res[mutant].items():
        print(f"{mutant}: {n}: {m}")
    assert not res[None], res[None]
    assert want <= set(res[mutant]), (mutant, sorted(res[mutant]))


def test_every_mutant_is_listed():
    assert set(REJECTS) == set(lo.MUTANTS) and len(lo.MUTANTS) == 12


@pytest.mark.parametrize("B,L,bm1", FWD_CASES)
def test_conditions_forward_cases(B, L, bm1):
    """Ambiguous share of the hidden h1 under 10 %, drifts of pre_l and s2 under 2 % of the rms, the between-tile
    term of the LayerNorm-1 merge at least 10 % of the variance where there are several partials."""
    c = lo.make_case(B, L, bm1, backward=False)
    led = lo.ConvLedger()
    for mode in ("fitted", "exact"):
        fails = []
        lo.forward_ref(c, mode, led, fails)
        assert not fails, fails
    if c["st1"].shape[1] > 1:
        share = lo.between_share(c["st1"], bm1, L)
        print(f"between-tile share of the variance {share:.3f}")
        assert share >= 0.10


@pytest.mark.parametrize("B,L", BWD_CASES)
def test_conditions_backward_cases(B, L):
    """Ambiguous shares of the hidden dpre (under 20 %) and h1 (under 10 %), drifts of dh1, dbl and dwl under 2 % of
    the rms, |m1| and |m2| of the order of rms(dxhat2); the constants are the stand-in's."""
    c = lo.make_case(B, L)
    kb = lo.bwd_inputs(c)
    cs = lo.play_backward(c, kb, "fitted")["consts"]
    led = lo.ConvLedger()
    for mode in ("fitted", "exact"):
        fails = []
        lo.backward_ref(c, kb, cs, mode, led, fails)
        assert not fails, fails
    rms = lo._rms(c["dh2"].to(F64) * c["g2"].to(F64))
    m1, m2 = float(cs[:, 2].abs().min()), float(cs[:, 3].abs().min())
    print(f"min |m1| {m1:.3f}  min |m2| {m2:.3f}  rms(dxhat2) {rms:.3f}")
    assert m1 > 0.25 * rms and m2 > 0.25 * rms
    if c["st1"].shape[1] > 1:
        assert lo.between_share(c["st1"], 128, L) >= 0.10


def _rel(a, b):
    return float((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm())


def test_present_inputs_hide_the_mutants():
    """With the inputs of tests/test_hip_ln_inflight.py (B = 33, L = 512, no ramp, dh2 = randn) the relative L2 error
    of a kernel without the m2 term, without the m1 term, or with truncating stores stays under that file's bounds
    (3e-2 backward, 1.5e-2 forward); with the inputs of make_case the first two exceed them tenfold."""
    FWD_TOL, BWD_TOL = 1.5e-2, 3e-2
    for plain in (True, False):
        c = lo.make_case(33, 512, plain=plain)
        kb = lo.bwd_inputs(c)
        good = lo.play_backward(c, kb, "exact", dt=F64, rounding=False)
        fwd = lo.play_forward(c, "exact", dt=F64, rounding=False)
        errs = {mu: _rel(lo.play_backward(c, kb, "exact", dt=F64, rounding=False, mutant=mu)["dh1"], good["dh1"])
                for mu in ("m2_term_dropped", "m1_term_dropped")}
        tr = lo.play_forward(c, "exact", mutant="bf16_truncate")
        errs["bf16_truncate"] = max(_rel(tr["s2"], fwd["s2"]), _rel(tr["pre_l"], fwd["pre_l"]))
        print(("present inputs: " if plain else "make_case:      ") + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        if plain:
            assert errs["m2_term_dropped"] < BWD_TOL / 4 and errs["m1_term_dropped"] < BWD_TOL / 4
            assert errs["bf16_truncate"] < FWD_TOL / 3
        else:
            assert errs["m2_term_dropped"] > 10 * BWD_TOL and errs["m1_term_dropped"] > 10 * BWD_TOL


def test_embedding_checks():
    """The embedding oracles accept the plain result and reject a truncated lookup and a dropped row."""
    e = lo.make_embed_case(1212)
    out = lo.rne_bf16(e["E"][e["tok"]])
    dE = e["dE0"].index_add(0, e["tok"].flip(0), e["dout"].to(F32).flip(0))
    lo.check_embed_fwd(e, out)
    lo.check_embed_bwd(e, dE)
    fails = []
    lo.check_embed_fwd(e, lo.trunc_bf16(e["E"][e["tok"]]), fails)
    lo.check_embed_bwd(e, dE - e["dout"][-1].to(F32) * (torch.arange(lo.V) == e["tok"][-1])[:, None], None, fails)
    assert {n for n, _ in fails} == {"embed_fwd.out", "embed_bwd.dE"}


def test_zero_e32_counter_example():
    """Why the yardstick of the tile means (and of the per-sample constants) is floored at half an fp32 ulp: a tile of
    one row is 128 bf16 values, whose fp32 sum can be exact in one order -- e32 = 0 -- and round once in another order
    of the same additions (on the GPU: (L = 33, B = 1), torch's sum exact, the kernel's 7.5e-9 off, against 16 x 0).
    Both are correct fp32 sums; with e32 = 0 the unfloored check demands the fp64 bits.  Both orders are written out
    here (explicit IEEE additions), so the example does not depend on how torch sums."""
    v = torch.zeros(1, C, dtype=F32)
    v[0, 0] = v[0, 1] = 2.0 ** -16                             # all three are bf16 values
    v[0, 2] = 256.0
    assert torch.equal(v, v.to(lo.BF16).to(F32))
    m64 = v.to(F64).mean(dim=1)
    fwd, rev = torch.zeros(1, dtype=F32), torch.zeros(1, dtype=F32)
    for i in range(C):
        fwd = fwd + v[:, i]                                    # 2^-15 + 256: 24 bits, exact
        rev = rev + v[:, C - 1 - i]                            # 256 + 2^-16 rounds back to 256, twice
    m32, alt = fwd / C, rev / C
    rows = torch.nonzero((m32.to(F64) == m64) & (alt.to(F64) != m64)).flatten()
    print(f"first channel first: err {float((m32.to(F64) - m64).abs()):.3e}; last channel first: "
          f"err {float((alt.to(F64) - m64).abs()):.3e}")
    assert rows.numel() == 1
    r = rows[:1]
    e = lo._e32(m32[r], m64[r])
    assert e == 0.0
    fails = []
    lo.check_elem("unfloored", alt[r], m64[r], e, None, None, fails)
    assert fails
    lo.check_elem("floored", alt[r], m64[r], max(e, lo.ulp_floor(m64[r])))
