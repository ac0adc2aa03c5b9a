"""CPU: the global-track oracles of tests/global_oracles.py are right on their own, so the GPU assertions of
tests/test_hip_global_exact.py mean something.

* With bf16 rounding switched off, the chained fp64 stages (forward and the hand-written backward) agree with
  fp64 ``torch.autograd`` of the plain block expression on all thirteen gradients.
* With rounding on, an fp32 torch transcription playing the kernel passes every stage check.
* Six altered transcriptions (``global_oracles.MUTANTS``) are each rejected at the smallest GPU shape."""
import pytest
import torch
import torch.nn.functional as F

import global_oracles as go
from global_oracles import EPS, make_case

F64 = torch.float64


def _reference64(g, vp, w1, b1, n1w, n1b, w2, b2, n2w, n2b, wp, wgl, bgl):
    """The ``_reference`` of tests/test_hip_global_track.py (the plain block expression), in fp64."""
    G = g.shape[1]
    z1 = g + F.gelu(g @ w1.t() + b1) + wp.mean() * vp.sum(dim=1)
    g1 = F.layer_norm(z1, (G,), n1w, n1b, eps=EPS)
    g2 = F.layer_norm(g1 + F.gelu(g1 @ w2.t() + b2), (G,), n2w, n2b, eps=EPS)
    gb = F.gelu(g2 @ wgl.t() + bgl) if wgl is not None else None
    return g2, gb


@pytest.mark.parametrize("B,G,NGL,TV,K", [(5, 256, 128, 3, 48), (19, 128, 0, 2, 1)])
def test_oracle_agrees_with_fp64_autograd(B, G, NGL, TV, K):
    """Rounding off: forward and all thirteen gradients against fp64 autograd.

    Bound: ``64 (3 G + B + TV) 2^-53 max|ref|`` per tensor -- three chained products of length G, a column sum
    over B rows and the TV partials are the reduction lengths, each term rounded to fp64 (2^-53 relative); 64
    covers the elementwise work between them (erf, exp, rsqrt, the LayerNorm's division by rstd ~ 1) and the
    error carried from one stage into the next.  No bf16 or fp32 quantity enters."""
    inp, par, dg2, dgb = make_case(B, G, NGL, TV, K)
    inp64 = {n: v.to(F64) for n, v in inp.items()}
    inp64["g_bf"] = inp64["g"]                                 # no rounding anywhere
    par64 = {n: (None if v is None else v.to(F64)) for n, v in par.items()}
    k = go.play_forward(inp64, par64, EPS, dt=F64, rounding=False)
    o, _ = go.play_backward(dg2.to(F64), None if dgb is None else dgb.to(F64), k, par64, inp64["wp"], dt=F64,
                            rounding=False)
    order = ["w1", "b1", "n1w", "n1b", "w2", "b2", "n2w", "n2b"]
    leaves = [inp64["g"], inp64["vpart"]] + [par64[n] for n in order] + [inp64["wp"]]
    if NGL:
        leaves += [par64["wgl"], par64["bgl"]]
    leaves = [t.clone().requires_grad_() for t in leaves]
    g2, gb = _reference64(*leaves[:11], *(leaves[11:] if NGL else (None, None)))
    loss = (g2 * dg2.to(F64)).sum() + ((gb * dgb.to(F64)).sum() if NGL else 0.0)
    grads = torch.autograd.grad(loss, leaves)
    mine = [o["dg"], o["dvs"].unsqueeze(1).expand(B, TV, G), o["dW1"], o["db1"], o["dn1w"], o["dn1b"], o["dW2"],
            o["db2"], o["dn2w"], o["dn2b"], o["dwp"]] + ([o["dWgl"], o["dbgl"]] if NGL else [])
    names = ["g", "vpart"] + order + ["wp"] + (["wgl", "bgl"] if NGL else [])
    assert len(mine) == len(grads) == (13 if NGL else 11)
    rel = 64 * (3 * G + B + TV) * 2.0 ** -53
    pairs = [("g2", k["g2"], g2.detach())] + ([("gb", k["gb"], gb.detach())] if NGL else [])
    pairs += [("d" + n, a, b) for n, a, b in zip(names, mine, grads)]
    for n, a, b in pairs:
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        print(f"{n:6s} err {err:.3e}  bound {rel * ref:.3e}")
        assert a.shape == b.shape and err <= rel * ref, (n, err, rel * ref)


SMALLEST = dict(B=1, G=256, NGL=0, TV=3, K=512)      # the smallest backward case of test_hip_global_exact.py


def _played(case, mutant=None):
    inp, par, dg2, dgb = case
    k = go.play_forward(inp, par, EPS, dt=torch.float32, rounding=True, mutant=mutant)
    o, stores = go.play_backward(dg2, dgb, k, par, inp["wp"], dt=torch.float32, rounding=True, mutant=mutant)
    got = {n: v for n, v in o.items() if not n.startswith("_")}
    got.update(stores)
    return k, got


@pytest.mark.parametrize("B,G,NGL,TV,K,off", [(1, 256, 0, 3, 48, False), (17, 512, 128, 5, 100, False),
                                              (37, 256, 128, 1, 64, True)])
def test_fp32_transcription_passes_every_stage(B, G, NGL, TV, K, off):
    """The reference alone (an fp32 torch transcription with the kernel's rounding points) is inside every
    condition of the helper, forward and backward."""
    case = make_case(B, G, NGL, TV, K, tile_offset=off)
    inp, par, dg2, dgb = case
    k, got = _played(case)
    led = go.Ledger()
    go.check_forward(inp, par, k, EPS, led)
    go.check_backward(dg2, dgb, k, par, inp["wp"], got, led)
    assert len(led.rows) >= 30


@pytest.mark.parametrize("mutant,where,match", [
    ("merge_no_between", "fwd", r"^r1"), ("rstd_bessel", "fwd", r"^r1"), ("residual_bf16", "fwd", r"^z2"),
    ("bf16_truncate", "fwd", r"g1_bf"), ("bf16_truncate", "bwd", r"^du2"), ("dwp_no_k", "bwd", r"^dwp"),
    ("colsum_clamped_row", "bwd", r"^(dn2w|dn2b|db2)")])
def test_helper_rejects_mutant(mutant, where, match):
    """Each altered transcription fails the stage it alters, at the smallest GPU shape (healthy: passes)."""
    assert mutant in go.MUTANTS
    case = make_case(**SMALLEST)
    inp, par, dg2, dgb = case
    k0, got0 = _played(case)
    go.check_forward(inp, par, k0, EPS)
    go.check_backward(dg2, dgb, k0, par, inp["wp"], got0)
    k, got = _played(case, mutant)
    with pytest.raises(AssertionError, match=match):
        if where == "fwd":
            go.check_forward(inp, par, k, EPS)
        else:
            go.check_backward(dg2, dgb, k0, par, inp["wp"], _played_bwd(case, k0, mutant))


def _played_bwd(case, k, mutant):
    """The mutant backward on a healthy forward, so the rejection is the backward's own."""
    inp, par, dg2, dgb = case
    o, stores = go.play_backward(dg2, dgb, k, par, inp["wp"], dt=torch.float32, rounding=True, mutant=mutant)
    got = {n: v for n, v in o.items() if not n.startswith("_")}
    got.update(stores)
    return got


def test_general_path_stages_on_cpu():
    """row_ln_fwd / row_ln_bwd / bias_gelu(_bwd) oracles: fp32 against fp64 inside the helper, and the row
    stage equal to the fused chain's first stage when fed the same pre-activation."""
    inp, par, dg2, _ = make_case(7, 384, 0, 5, 48)
    u = inp["g_bf"].float() @ go.rne_bf16(par["w1"]).float().t()
    o64 = go.row_ln_fwd(u, par["b1"], inp["g"], inp["vpart"], inp["wp"], par["n1w"], par["n1b"], EPS, F64)
    o32 = go.row_ln_fwd(u, par["b1"], inp["g"], inp["vpart"], inp["wp"], par["n1w"], par["n1b"], EPS, torch.float32)
    for n in ("vsum", "rstd", "xhat", "out"):
        go.check(n, o32[n], o64[n], o32[n], 0.0)
    z1 = go.st_z1(inp["g"], u.to(F64) + par["b1"].to(F64), o64["vsum"], inp["wp"], F64)
    m, r = go.st_row_stats(z1, EPS, F64)
    assert torch.allclose(o64["out"], go.st_ln(z1, m, r, par["n1w"], par["n1b"], F64)[1], rtol=0, atol=1e-13)
    b64 = go.row_ln_bwd(dg2, o64["xhat"].float(), o64["rstd"].float(), par["n1w"], u, par["b1"], o64["vsum"].float(),
                        inp["wp"], F64)
    z = (inp["g"].to(F64)).requires_grad_()
    uu = u.to(F64).requires_grad_()
    zz = z + F.gelu(uu + par["b1"].to(F64)) + inp["wp"].to(F64).mean() * inp["vpart"].to(F64).sum(1)
    out = F.layer_norm(zz, (384,), par["n1w"].to(F64), par["n1b"].to(F64), eps=EPS)
    dres, du = torch.autograd.grad((out * dg2.to(F64)).sum(), [z, uu])
    # xhat / rstd were rounded to fp32 on the way in: fp32-level agreement
    assert float((b64["dres"] - dres).abs().max()) <= 1e-5 and float((b64["du"] - du).abs().max()) <= 1e-5
    g64 = go.bias_gelu_bwd(dg2, u, par["b1"], F64)
    assert torch.allclose(g64["dbias"], g64["du"].sum(0)) and g64["du"].shape == u.shape
    assert torch.allclose(go.bias_gelu(u, par["b1"], F64), F.gelu(u.to(F64) + par["b1"].to(F64)), rtol=0, atol=1e-14)
