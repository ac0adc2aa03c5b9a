"""GPU numerics of the first block's token-table conv forward (csrc/conv_tok.hip, ``pbx_conv_fwd_tok``).

The oracle is float64 from the bf16-rounded weights and embedding: ``pre`` of both convolutions, then ``s1`` and
GELU' through a float64 GELU of the build's form (fitted logistic or erf).  The yardstick is the kernel it
replaces, ``pbx_conv_fwd3t`` (1,152 sequential products per ``pre``), on the same inputs: the new kernel's max
abs error may exceed the yardstick's by at most one bf16 step of the output's magnitude, and its outputs may
differ from the yardstick's only in the rare elements whose fp32 ``pre`` sits on a bf16 rounding boundary.

Shapes: one tile with both sequence edges inside the +-20 halo; a tile boundary crossed by the dilation-5 taps;
more (tile, half) units than workgroups on 256 CUs (the persistent walk wraps); L = 200, which the kernel
declines (the dispatcher falls back to ``pbx_conv_fwd3t``, bitwise).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

V, C, KS, DIL = 26, 128, 9, 5
SHAPES = [(3, 128), (3, 256), (40, 512)]
# Share of pre-derived output elements (s1, both GELU' images) allowed to differ from pbx_conv_fwd3t.  Only the
# order of the fp32 sum inside pre differs: the two sums are a few fp32 ulps (~2^-22 relative) apart, a bf16
# rounding boundary comes every 2^-8 relative, so a pre flips with probability ~1e-4 and an s1 element (two
# pre's) about twice as often at most.  Measured shares (profiles/r9/conv_tok_agreement.txt) are 2.7e-5 .. 3.0e-5;
# the cap leaves a 10x margin over the largest (44 elements at the smallest shape, where 4 differ) and stays
# three orders of magnitude under what one wrong tap or table row gives (nearly every element).
DIFF_CAP = 3e-4


def _gelu64(x):
    """(GELU, GELU') in float64 in the form of the loaded build (ops/csrc/common.h)."""
    from proteinbert_pytorch_replication_amd.ops import _lib
    if _lib.gelu_mode() == "exact":
        Phi = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return x * Phi, Phi + x * phi
    t = x * x
    s = 1.0 / (1.0 + torch.exp2((t * -0.10053117 - 2.3073633) * x))
    return x * s, s + x * s * (1.0 - s) * (1.59934236 + 0.20904868 * t)


def _mean_var(st, bm):
    """Per-sample (mean, variance) from (mean, M2) partials of bm x 128 elements each (Chan merge, float64)."""
    st = st.double()
    n = float(bm * C)
    mean = st[..., 0].mean(dim=1)
    M2 = st[..., 1].sum(dim=1) + n * ((st[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    return mean, M2 / (n * st.shape[1])


def _tokens(B, L):
    tok = torch.randint(0, V, (B, L), device="cuda")
    for b in range(B):
        # every token value in every sample's two 20-position edges (the wide conv's halo), shifted per sample
        edge = (torch.arange(20, device="cuda") + 7 * b) % V
        tok[b, :20] = edge
        tok[b, L - 20:] = (edge + 13) % V
    tok[0, 20:20 + V] = torch.arange(V, device="cuda")
    assert set(tok.flatten().tolist()) == set(range(V))
    return tok.contiguous()


def _run(name, c, store=True):
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.ops import local_track as lt
    B, L = c["tok"].shape
    st = _lib.stream_ptr(torch.device("cuda"))
    o = [torch.full((B, L, C), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    gdn, gdw = (o[0], o[1]) if store else (None, None)
    if name == "parent":
        T1, bm = (L + 127) // 128, 128
        st1 = torch.empty(B, T1, 2, device="cuda")
        _lib.call("pbx_conv_fwd3t", c["tok"].data_ptr(), c["eb"].data_ptr(), c["wpn"].data_ptr(), c["wpw"].data_ptr(),
                  c["bn"].data_ptr(), c["bw"].data_ptr(), c["gb"].data_ptr(), lt._p(gdn), lt._p(gdw), o[2].data_ptr(),
                  st1.data_ptr(), B, L, KS, DIL, st)
    else:
        st1, T1, bm = lt.conv_fwd_first(c["tok"], c["eb"], c["wpn"], c["wpw"], c["bn"], c["bw"], c["gb"], gdn, gdw,
                                        o[2], KS, DIL, st)
    torch.cuda.synchronize()
    return {"gdn": o[0], "gdw": o[1], "s1": o[2], "st": st1, "bm": bm}


@functools.lru_cache(maxsize=None)
def case(B, L):
    """Inputs, float64 oracle, the yardstick's and the new kernel's outputs of one shape (computed once)."""
    from proteinbert_pytorch_replication_amd.ops.local_track import pack_conv
    torch.manual_seed(1000 * B + L)
    dev = "cuda"
    c = {"tok": _tokens(B, L), "eb": torch.randn(V, C, device=dev).to(torch.bfloat16).contiguous()}
    wn, ww = torch.randn(C, C, KS, device=dev) * 0.05, torch.randn(C, C, KS, device=dev) * 0.05
    c["bn"], c["bw"], c["gb"] = torch.randn(C, device=dev), torch.randn(C, device=dev), torch.randn(B, C, device=dev)
    (c["wpn"], _), (c["wpw"], _) = pack_conv(wn), pack_conv(ww)
    x = c["eb"].double()[c["tok"]]                                   # [B, L, C]
    pre = []
    for w, b, d in ((wn, c["bn"], 1), (ww, c["bw"], DIL)):
        wb = w.to(torch.bfloat16).double()
        xp = torch.nn.functional.pad(x, (0, 0, 4 * d, 4 * d))
        pre.append(b.double() + sum(xp[:, k * d:k * d + L] @ wb[:, :, k].t() for k in range(KS)))
    (gn, dn), (gw, dw) = _gelu64(pre[0]), _gelu64(pre[1])
    s1 = x + gn + gw + c["gb"].double()[:, None, :]
    mean = s1.mean(dim=(1, 2))
    c["oracle"] = {"s1": s1, "gdn": dn, "gdw": dw, "mean": mean,
                   "var": ((s1 - mean[:, None, None]) ** 2).mean(dim=(1, 2))}
    c["parent"] = _run("parent", c)
    c["new"] = _run("new", c)
    return c


def _errors(out, oracle):
    mean, var = _mean_var(out["st"], out["bm"])
    e = {k: (out[k].double() - oracle[k]).abs().max().item() for k in ("s1", "gdn", "gdw")}
    e["mean"] = (mean - oracle["mean"]).abs().max().item()
    e["var"] = (var - oracle["var"]).abs().max().item()
    return e


@pytest.mark.parametrize("B,L", SHAPES)
def test_takes_the_table_kernel(B, L):
    from proteinbert_pytorch_replication_amd.ops.local_track import conv_tok_ok
    assert conv_tok_ok(B, L, KS, DIL, V)
    assert case(B, L)["new"]["bm"] == 4 and case(B, L)["new"]["st"].shape == (B, L // 4, 2)
    for k in ("s1", "gdn", "gdw"):
        assert torch.isfinite(case(B, L)["new"][k].float()).all()    # every element written


@pytest.mark.parametrize("B,L", SHAPES)
def test_error_within_one_bf16_step_of_the_parent(B, L):
    c = case(B, L)
    en, ep = _errors(c["new"], c["oracle"]), _errors(c["parent"], c["oracle"])
    for k in ("s1", "gdn", "gdw", "mean", "var"):
        mag = c["oracle"][k].abs().max().item()
        step = 2.0 ** (math.floor(math.log2(mag)) - 7)               # one bf16 step at the output's magnitude
        print(f"B={B} L={L} {k}: new {en[k]:.3e} parent {ep[k]:.3e} bf16 step {step:.3e}")
        assert en[k] <= ep[k] + step, (k, en[k], ep[k], step)


@pytest.mark.parametrize("B,L", SHAPES)
def test_agrees_with_the_parent_but_for_rounding_boundaries(B, L):
    c = case(B, L)
    diff = sum((c["new"][k] != c["parent"][k]).sum().item() for k in ("s1", "gdn", "gdw"))
    share = diff / (3 * B * L * C)
    print(f"B={B} L={L}: {diff} of {3 * B * L * C} elements differ from pbx_conv_fwd3t, share {share:.3e}")
    assert share < DIFF_CAP


def test_declined_length_falls_back_bitwise():
    from proteinbert_pytorch_replication_amd.ops.local_track import conv_tok_ok
    B, L = 2, 200
    assert not conv_tok_ok(B, L, KS, DIL, V)
    c = case(B, L)
    assert c["new"]["bm"] == 128
    for k in ("s1", "gdn", "gdw", "st"):
        assert torch.equal(c["new"][k], c["parent"][k])


@pytest.mark.parametrize("B,L", SHAPES)
def test_inference_variant_and_repeatability(B, L):
    c = case(B, L)
    again = _run("new", c)
    for k in ("s1", "gdn", "gdw", "st"):
        assert torch.equal(again[k], c["new"][k])
    inf = _run("new", c, store=False)
    assert torch.equal(inf["s1"], c["new"]["s1"]) and torch.equal(inf["st"], c["new"]["st"])
    assert torch.isnan(inf["gdn"].float()).all() and torch.isnan(inf["gdw"].float()).all()   # not written
