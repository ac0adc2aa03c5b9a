"""GPU numerics of the LayerNorm-1 / local-MLP forward and the LayerNorm-2 / MLP backward kernels called
directly (``pbx_ln_linear_fwd``, ``pbx_ln2_linear_bwd``), at the batch sizes where their load rings and
dropped stores can go wrong.

Both kernels keep the next samples' rows in flight while the current ones are computed: the forward
D = ``pbx_ln_fwd_ring()`` samples per workgroup, the backward one 16-sample chunk.  The backward's loads past
the last sample or the last position read a clamped address and are masked at use; its stores of rows past L
(and of samples past the workgroup's range) are buffer stores with an out-of-range offset.  So the cases are
chosen by the number of samples ONE workgroup walks (computed from the device's CU count as the launchers
do): 1, D - 1, D, D + 1 and 2 D + 1 with uneven groups, a last position tile with 26 (one) valid rows, a
last position pair with one position, and sample splits.

Oracle: the same math in fp32 torch, with the error bounds tests/test_hip_local_track.py applies to the
block these kernels are part of (relative L2 error 1.5e-2 forward, 3e-2 backward).  Every case runs twice:
the outputs with a single writer (s2, pre_l, st2; dh1, sums1) must repeat bitwise.  Outputs carry a guard
of rows behind them that no store may touch.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from proteinbert_pytorch_replication_amd.ops import _lib

pytestmark = pytest.mark.gpu

CH, PB, BM1, EPS = 128, 32, 128, 1e-5
FWD_TOL, BWD_TOL = 1.5e-2, 3e-2        # tests/test_hip_local_track.py: forward / backward of the local block
GUARD = 64                             # rows of 128 behind every [B, L, 128] output
SENT = -7.0                            # guard fill (exact in bf16)
BWD_DEPTH = 1                          # chunks of 16 samples the backward prefetches ahead


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def fwd_groups(B, L):
    """ln_groups of csrc/ln.hip: sample groups of the forward's grid."""
    tp = (L + PB - 1) // PB
    g = (2 * cus() + tp - 1) // tp
    return max(1, min(g, B))


def walked(B, g):
    return sorted({B * (y + 1) // g - B * y // g for y in range(g)})


def tile_stats(x, bm):
    """(mean, M2) per tile of bm positions x 128 channels: [B, ceil(L / bm), 2] fp32."""
    B, L, _ = x.shape
    out = []
    for t in range((L + bm - 1) // bm):
        v = x[:, t * bm:(t + 1) * bm].reshape(B, -1).float()
        m = v.mean(1)
        out.append(torch.stack([m, ((v - m[:, None]) ** 2).sum(1)], 1))
    return torch.stack(out, 1).contiguous()


def guarded(B, L, dtype=torch.bfloat16):
    buf = torch.full((B * L + GUARD, CH), SENT, dtype=dtype, device="cuda")
    return buf, buf[:B * L].view(B, L, CH)


def guard_ok(buf, B, L):
    return bool((buf[B * L:] == SENT).all().item())


@functools.lru_cache(maxsize=None)
def case_data(L, Bmax):
    """Inputs and the fp32 oracle of the forward for Bmax samples (LayerNorm is per sample: a case with
    fewer samples uses the leading slice), computed once per (L, Bmax) and left unchanged."""
    gen = torch.Generator(device="cuda").manual_seed(1000 + L)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)   # noqa: E731
    d = {}
    d["s1"] = (rn(Bmax, L, CH) * 1.3 + 0.2).to(torch.bfloat16)
    d["g1"], d["be1"] = 1.0 + 0.2 * rn(L, CH), 0.2 * rn(L, CH)
    d["g2"] = 1.0 + 0.2 * rn(L, CH)
    d["wl"] = (rn(CH, CH) / CH ** 0.5).to(torch.bfloat16)
    d["bl"] = 0.1 * rn(CH)
    d["st1"] = tile_stats(d["s1"], BM1)
    h1 = F.layer_norm(d["s1"].float(), (L, CH), d["g1"], d["be1"], EPS)
    pre = h1 @ d["wl"].float().t() + d["bl"]
    d["h1"], d["pre"], d["s2"] = h1, pre, h1 + F.gelu(pre)
    d["st2"] = tile_stats(d["s2"], PB)
    # backward inputs: the forward's tensors as the kernels store them, and an upstream gradient
    d["pre_b"], d["s2_b"] = pre.to(torch.bfloat16), d["s2"].to(torch.bfloat16)
    d["st2_b"] = tile_stats(d["s2_b"], PB)
    d["dh2"] = rn(Bmax, L, CH).to(torch.bfloat16)
    return d


def run_fwd(d, B, L, with_pre=True):
    s1 = d["s1"][:B].contiguous()
    st1 = d["st1"][:B].contiguous()
    T1, T2 = st1.shape[1], (L + PB - 1) // PB
    pbuf, pre = guarded(B, L)
    sbuf, s2 = guarded(B, L)
    st2 = torch.full((B * T2 + GUARD, 2), SENT, dtype=torch.float32, device="cuda")
    _lib.call("pbx_ln_linear_fwd", s1.data_ptr(), st1.data_ptr(), T1, BM1, d["g1"].data_ptr(), d["be1"].data_ptr(),
              d["wl"].data_ptr(), d["bl"].data_ptr(), pbuf.data_ptr() if with_pre else None, sbuf.data_ptr(),
              st2.data_ptr(), B, L, EPS, _lib.stream_ptr(s1.device))
    torch.cuda.synchronize()
    assert guard_ok(sbuf, B, L) and guard_ok(pbuf, B, L), "a store landed behind the output"
    assert bool((st2[B * T2:] == SENT).all().item())
    return pre, s2, st2[:B * T2].view(B, T2, 2)


def fwd_cases():
    """(L, samples one workgroup walks) -> B, from the device's group count; ids name the walk."""
    D = _lib.lib().pbx_ln_fwd_ring()
    out = []
    for L in (4096, 4090):
        g = fwd_groups(10 ** 6, L)
        # even groups of 1, D - 1, D and 2 D + 1 samples; D / D + 1 and 2 D / 2 D + 1 samples in uneven groups
        for B in sorted({g, g * max(D - 1, 1), g * D, g * D + 1, g * (2 * D + 1) - 1, g * (2 * D + 1)}):
            out.append((L, B))
    return D, out


def test_forward_walks_cover_the_ring():
    """The batch sizes below make a workgroup walk 1, D - 1, D, D + 1 and 2 D + 1 samples on this device."""
    D, cases = fwd_cases()
    seen = set()
    for L, B in cases:
        seen |= set(walked(B, fwd_groups(B, L)))
    print(f"D={D} CUs={cus()} cases={cases} walks={sorted(seen)}")
    assert {1, max(D - 1, 1), D, D + 1, 2 * D + 1} <= seen


@pytest.mark.parametrize("L", [4096, 4090])
def test_ln_linear_fwd_ring(L):
    D, cases = fwd_cases()
    Bs = [B for ll, B in cases if ll == L]
    d = case_data(L, max(Bs))
    for B in Bs:
        pre, s2, st2 = run_fwd(d, B, L)
        pre_b, s2_b, st2_b = run_fwd(d, B, L)
        e_pre, e_s2, e_st = rel(pre, d["pre"][:B]), rel(s2, d["s2"][:B]), rel(st2, d["st2"][:B])
        # the partials are those of the values the kernel stored (fp32 sums of 32 x 128 values of O(1):
        # a relative error of some 1e-6 each, 1e-3 is three orders above it)
        e_own = rel(st2, tile_stats(s2, PB))
        print(f"L={L} B={B} walks={walked(B, fwd_groups(B, L))} D={D}: rel pre {e_pre:.2e} s2 {e_s2:.2e} "
              f"st2 {e_st:.2e} st2-vs-stored {e_own:.2e}")
        assert e_pre < FWD_TOL and e_s2 < FWD_TOL and e_st < FWD_TOL
        assert e_own < 1e-3
        assert torch.equal(pre, pre_b) and torch.equal(s2, s2_b) and torch.equal(st2, st2_b), "not repeatable"


def test_ln_linear_fwd_second_tile_of_one_row():
    """B = 1, L = 33: the second position tile has one valid row; without pre_l (no backward) s2 and st2 are
    the same bits."""
    L, B = 33, 1
    d = case_data(L, B)
    pre, s2, st2 = run_fwd(d, B, L)
    pre_b, s2_b, st2_b = run_fwd(d, B, L)
    _, s2_n, st2_n = run_fwd(d, B, L, with_pre=False)
    e_pre, e_s2, e_st = rel(pre, d["pre"]), rel(s2, d["s2"]), rel(st2, d["st2"])
    print(f"L={L} B={B}: rel pre {e_pre:.2e} s2 {e_s2:.2e} st2 {e_st:.2e}")
    assert e_pre < FWD_TOL and e_s2 < FWD_TOL and e_st < FWD_TOL
    assert torch.equal(pre, pre_b) and torch.equal(s2, s2_b) and torch.equal(st2, st2_b), "not repeatable"
    assert torch.equal(s2, s2_n) and torch.equal(st2, st2_n)


# ----------------------------------------------------------------------------------------------------------
def ref_bwd(d, B, L):
    """fp32 oracle of pbx_ln2_linear_bwd on the first B samples (inputs as the kernel reads them)."""
    s1, s2, pre, dh2 = (d[k][:B].float() for k in ("s1", "s2_b", "pre_b", "dh2"))
    g1, be1, g2, wl = d["g1"], d["be1"], d["g2"], d["wl"].float()

    def xhat(x):
        v = x.reshape(B, -1)
        m, var = v.mean(1), v.var(1, unbiased=False)
        return (x - m[:, None, None]) * torch.rsqrt(var + EPS)[:, None, None]

    xh2, xh1 = xhat(s2), xhat(s1)
    dxh2 = dh2 * g2
    m1 = dxh2.reshape(B, -1).mean(1)[:, None, None]
    m2 = (dxh2 * xh2).reshape(B, -1).mean(1)[:, None, None]
    rstd2 = torch.rsqrt(s2.reshape(B, -1).var(1, unbiased=False) + EPS)[:, None, None]
    ds2 = rstd2 * (dxh2 - m1 - xh2 * m2)
    gp = 0.5 * (1.0 + torch.erf(pre / 2 ** 0.5)) + pre * torch.exp(-0.5 * pre * pre) / (2 * torch.pi) ** 0.5
    dpre = ds2 * gp
    dh1 = ds2 + dpre @ wl
    h1 = xh1 * g1 + be1
    dxh1 = dh1 * g1
    TS1 = (L + 1) // 2
    pad = torch.zeros(B, 2 * TS1 - L, CH, device=s1.device)
    pairs = lambda x: torch.cat([x, pad], 1).reshape(B, TS1, 2 * CH).sum(2)   # noqa: E731
    return {"dh1": dh1, "sums1": torch.stack([pairs(dxh1), pairs(dxh1 * xh1)], 2),
            "dg2": (dh2 * xh2).sum(0), "db2": dh2.sum(0), "dg1": (dh1 * xh1).sum(0), "db1": dh1.sum(0),
            "dwl": dpre.reshape(-1, CH).t() @ h1.reshape(-1, CH), "dbl": dpre.reshape(-1, CH).sum(0)}


def run_bwd(d, B, L, det):
    dev = d["s1"].device
    s1, s2, pre, dh2 = (d[k][:B].contiguous() for k in ("s1", "s2_b", "pre_b", "dh2"))
    st1, st2 = d["st1"][:B].contiguous(), d["st2_b"][:B].contiguous()
    T1, TA, TS1 = st1.shape[1], (L + 31) // 32, (L + 1) // 2
    # LN2 backward partials per 32-position tile, as the pool backward writes them
    v = s2.float().reshape(B, -1)
    xh2 = (s2.float() - v.mean(1)[:, None, None]) * torch.rsqrt(v.var(1, unbiased=False) + EPS)[:, None, None]
    dxh2 = dh2.float() * d["g2"]
    padr = TA * 32 - L
    tiles = lambda x: F.pad(x, (0, 0, 0, padr)).reshape(B, TA, 32 * CH).sum(2)   # noqa: E731
    sums2 = torch.stack([tiles(dxh2), tiles(dxh2 * xh2)], 2).contiguous()
    consts = torch.empty((B, 8), dtype=torch.float32, device=dev)
    dgb = torch.empty((B, CH), dtype=torch.float32, device=dev)
    dbuf, dh1 = guarded(B, L)
    sums1 = torch.full((B * TS1 + GUARD, 2), SENT, dtype=torch.float32, device=dev)
    acc = {k: torch.zeros(s, dtype=torch.float32, device=dev)
           for k, s in (("dg2", (L, CH)), ("db2", (L, CH)), ("dg1", (L, CH)), ("db1", (L, CH)), ("dwl", (CH, CH)),
                        ("dbl", (CH,)))}
    rows = _lib.lib().pbx_ln2_bwd_slab_rows(B, L, det)
    slab = torch.empty(rows * (CH * CH + CH), dtype=torch.float32, device=dev)
    _lib.call("pbx_ln2_linear_bwd", dh2.data_ptr(), s2.data_ptr(), st2.data_ptr(), sums2.data_ptr(), TA,
              d["g2"].data_ptr(), pre.data_ptr(), s1.data_ptr(), st1.data_ptr(), T1, BM1, d["g1"].data_ptr(),
              d["be1"].data_ptr(), d["wl"].data_ptr(), consts.data_ptr(), dbuf.data_ptr(), sums1.data_ptr(),
              acc["dg2"].data_ptr(), acc["db2"].data_ptr(), acc["dg1"].data_ptr(), acc["db1"].data_ptr(),
              acc["dwl"].data_ptr(), acc["dbl"].data_ptr(), dgb.data_ptr(), B, L, EPS, slab.data_ptr(), rows, det, 1, 0,
              _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert guard_ok(dbuf, B, L), "a dh1 store landed behind the output"
    assert bool((sums1[B * TS1:] == SENT).all().item()), "a sums1 store landed behind the output"
    acc["dh1"], acc["sums1"] = dh1, sums1[:B * TS1].view(B, TS1, 2)
    return acc


BWD_CASES = [(512, 1, 0), (512, 16, 0), (512, 17, 0), (512, 16 * BWD_DEPTH + 1, 0),
             (512, 16 * (BWD_DEPTH + 1) + 5, 0), (511, 33, 0), (64, 80, 0), (512, 33, 1)]


@pytest.mark.parametrize("L,B,det", sorted(set(BWD_CASES)))
def test_ln2_linear_bwd_chunks(L, B, det):
    """L = 512: one workgroup per position pair walks every sample on a 256-CU device (1 sample, one chunk,
    one chunk + 1, D chunks + 1 and D + 1 chunks + 5 with D = BWD_DEPTH); L = 511: the last pair has one
    position; L = 64, B = 80: sample splits of 16; det = 1: the deterministic grid."""
    d = case_data(L, max(b for ll, b, _ in BWD_CASES if ll == L))
    ref = ref_bwd(d, B, L)
    a, b = run_bwd(d, B, L, det), run_bwd(d, B, L, det)
    errs = {k: rel(a[k], ref[k]) for k in ("dh1", "sums1", "dg2", "db2", "dg1", "db1", "dwl", "dbl")}
    print(f"L={L} B={B} det={det}: " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < BWD_TOL, f"{k}: rel err {e:.3e}"
    assert torch.equal(a["dh1"], b["dh1"]) and torch.equal(a["sums1"], b["sums1"]), "dh1 / sums1 not repeatable"
    if det:
        for k in ("dg2", "db2", "dg1", "db1", "dwl", "dbl"):
            assert torch.equal(a[k], b[k]), f"{k} not repeatable in the deterministic mode"
