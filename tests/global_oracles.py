"""Stage-wise oracles (torch only, float64 by default) for the global-track kernels: the column-split
forward of ``ops/csrc/glob3.hip``, the one-launch backward and the fragment packer of ``ops/csrc/glob2.hip``
and the row LayerNorm / bias-GELU kernels of ``ops/csrc/glob.hip``.

The kernels store every intermediate, so each stage is evaluated on its own from the tensors the kernel
itself stored for the stage before (the ``k`` dictionaries below).  The only legitimate difference between a
stored tensor and its oracle is then fp32 arithmetic -- no bf16 rounding has to be absorbed by a tolerance.

* Every stage function takes ``dt``: ``torch.float64`` gives the oracle X_64, ``torch.float32`` the yardstick
  X_32 (the same stage from the same inputs in plain fp32 torch ops, independent of the kernel's order).
* :func:`check` asserts ``max |X_k - X_64| <= 16 * max |X_32 - X_64| + gelu_term``; ``gelu_term`` is the
  documented bound of the A&S 7.1.26 erf core of ``common.h`` (1.5e-7) times the magnitude it multiplies,
  and only outputs that pass through a GELU / GELU' carry it.  :func:`check_bf16` is the form for a bf16
  store: half a bf16 ulp of the fp64 value plus the fp32 slack of the value before rounding.
* :func:`play_forward` / :func:`play_backward` chain the stages on their own outputs ("playing the kernel").
  With ``rounding=False`` in fp64 they are the plain block expression (validated against autograd in
  tests/test_global_oracles.py); in fp32 with rounding on they are a stand-in kernel, and with a ``mutant``
  name a deliberately wrong one that the checks must reject.
"""
import math

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
CT = 64                  # columns per LayerNorm partial (glob3.hip)
RB = 16                  # rows per workgroup (glob2.hip / glob3.hip)
MARGIN = 16.0            # the project's margin over the fp32 torch error (summation order differs)
GELU_CORE = 1.5e-7       # |erf error| of the A&S 7.1.26 core (common.h)
BF16_BITS = 8            # significand bits of bf16, the hidden one included

EPS = 1e-5               # global_track.LN_EPS

MUTANTS = ("merge_no_between", "rstd_bessel", "dwp_no_k", "residual_bf16", "colsum_clamped_row", "bf16_truncate")


# ---- test inputs --------------------------------------------------------------------------------------
def make_case(B, G, NGL, TV, K, tile_offset=False, seed=5, dev="cpu"):
    """Inputs and parameters at the scales of tests/test_hip_global_track.py (fp32)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).to(dev)  # noqa: E731
    par = dict(w1=rn(G, G, sc=G ** -0.5), b1=rn(G, sc=0.1), n1w=1 + rn(G, sc=0.1), n1b=rn(G, sc=0.1),
               w2=rn(G, G, sc=G ** -0.5), b2=rn(G, sc=0.1), n2w=1 + rn(G, sc=0.1), n2b=rn(G, sc=0.1))
    wp = rn(K)
    par["wgl"], par["bgl"] = (rn(NGL, G, sc=G ** -0.5), rn(NGL, sc=0.1)) if NGL else (None, None)
    g = rn(B, G)
    if tile_offset:      # the between-tile term dominates the row variance
        g = g + 3.0 * (torch.arange(G, device=dev) // CT).float()
    inp = dict(g=g, g_bf=g.to(BF16), vpart=rn(B, TV, G, sc=0.05), wp=wp)
    dg2 = rn(B, G)
    dgb = rn(B, NGL) if NGL else None
    return inp, par, dg2, dgb


# ---- number formats ---------------------------------------------------------------------------------
def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """RNE bf16 of an fp32 tensor (what ``f2bf`` does)."""
    return x.to(F32).to(BF16)


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 by dropping the low 16 bits (the ``bf16_truncate`` mutant)."""
    bits = x.to(F32).contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(F32).to(BF16)


def bf16_half_ulp(x: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp at every element of an fp64 tensor: 2^(floor(log2 |x|) - 8), i.e. between 2^-9 |x| (top of
    a binade) and 2^-8 |x| (bottom).  A correctly rounded store is always within this of x (2^-9 |x| alone is
    not enough: 2.3194 rounds to 2.3125, 6.9e-3 away, while 2^-9 |x| = 4.5e-3); truncation errs by up to twice it."""
    _, e = torch.frexp(x.to(F64).abs())                     # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 1 - BF16_BITS)


def wimg(w: torch.Tensor, dt=F64, rounding: bool = True) -> torch.Tensor:
    """The bf16 image of an fp32 weight, promoted to ``dt`` (``rounding=False``: the weight itself)."""
    return (rne_bf16(w) if rounding else w).to(dt)


def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    cdf = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    return cdf + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


# ---- forward stages -----------------------------------------------------------------------------------
def st_vsum(vpart, dt=F64):
    return vpart.to(dt).sum(dim=1)


def st_pre(x_bf, w, b, dt=F64, rounding=True):
    """x_bf @ bf16(W)^T + b."""
    return x_bf.to(dt) @ wimg(w, dt, rounding).t() + b.to(dt)


def st_z1(g, pre1, vsum, wp, dt=F64):
    return g.to(dt) + gelu(pre1.to(dt)) + wp.to(dt).mean() * vsum.to(dt)


def st_part(z, dt=F64):
    """[B, G / 64, 2]: (mean, M2) of every 64-column tile."""
    B, G = z.shape
    zt = z.to(dt).reshape(B, G // CT, CT)
    m = zt.mean(dim=-1)
    return torch.stack([m, ((zt - m[..., None]) ** 2).sum(dim=-1)], dim=-1)


def st_merge(part, G, eps, dt=F64, mutant=None):
    """Chan merge of the partials: (mean [B], rstd [B])."""
    p = part.to(dt)
    m = p[..., 0].mean(dim=1)
    M2 = p[..., 1].sum(dim=1)
    if mutant != "merge_no_between":
        M2 = M2 + (CT * (p[..., 0] - m[:, None]) ** 2).sum(dim=1)
    den = G - 1 if mutant == "rstd_bessel" else G
    return m, torch.rsqrt(M2 / den + eps)


def st_row_stats(z, eps, dt=F64):
    """Plain full-row (mean [B], rstd [B]) -- what the merged partials must reproduce."""
    z = z.to(dt)
    m = z.mean(dim=1)
    return m, torch.rsqrt(((z - m[:, None]) ** 2).mean(dim=1) + eps)


def st_ln(z, mean, rstd, nw, nb, dt=F64):
    xh = (z.to(dt) - mean.to(dt)[:, None]) * rstd.to(dt)[:, None]
    return xh, xh * nw.to(dt) + nb.to(dt)


def st_z2(o1, pre2, dt=F64):
    return o1.to(dt) + gelu(pre2.to(dt))


def forward_stages(inp, par, k, eps, dt=F64):
    """Every output of the fused forward from the kernel-stored inputs of its stage.

    inp: g, g_bf, vpart, wp.  par: w1 b1 n1w n1b w2 b2 n2w n2b [wgl bgl].  k: the kernel's stored tensors.
    Returns name -> tensor (``dt``).  The ``*_plain`` entries are the direct check of the merge: in fp64 the plain
    full-row statistics of the stored z, in fp32 (the yardstick) per-tile partials and their merge, both from z."""
    G = inp["g"].shape[1]
    o = {}
    o["vsum"] = st_vsum(inp["vpart"], dt)
    o["pre1"] = st_pre(inp["g_bf"], par["w1"], par["b1"], dt)
    o["z1"] = st_z1(inp["g"], k["pre1"], k["vsum"], inp["wp"], dt)
    p1 = st_part(k["z1"], dt)
    o["part1_mean"], o["part1_M2"] = p1[..., 0], p1[..., 1]
    m1, o["r1"] = st_merge(k["part1"], G, eps, dt)
    o["xh1"], o["o1"] = st_ln(k["z1"], m1, o["r1"], par["n1w"], par["n1b"], dt)
    m1p, o["r1_plain"] = st_row_stats(k["z1"], eps, dt) if dt == F64 else st_merge(p1, G, eps, dt)
    o["xh1_plain"] = st_ln(k["z1"], m1p, o["r1_plain"], par["n1w"], par["n1b"], dt)[0]
    o["pre2"] = st_pre(k["g1_bf"], par["w2"], par["b2"], dt)
    o["z2"] = st_z2(o["o1"], k["pre2"], dt)
    p2 = st_part(k["z2"], dt)
    o["part2_mean"], o["part2_M2"] = p2[..., 0], p2[..., 1]
    m2, o["r2"] = st_merge(k["part2"], G, eps, dt)
    o["xh2"], o["g2"] = st_ln(k["z2"], m2, o["r2"], par["n2w"], par["n2b"], dt)
    m2p, o["r2_plain"] = st_row_stats(k["z2"], eps, dt) if dt == F64 else st_merge(p2, G, eps, dt)
    o["xh2_plain"] = st_ln(k["z2"], m2p, o["r2_plain"], par["n2w"], par["n2b"], dt)[0]
    if par.get("wgl") is not None:
        o["pregl"] = st_pre(k["g2_bf"], par["wgl"], par["bgl"], dt)
        o["gb"] = gelu(k["pregl"].to(dt))
    return o


# ---- backward stages ----------------------------------------------------------------------------------
def st_ln_bwd(dy, xh, r, nw, pre, dt=F64, rows=None):
    """LayerNorm + GELU backward of one stage.  Returns ds, du (unrounded), dnw, dnb, db and |ds| column
    sums (the magnitude the GELU' error multiplies in db).  ``rows``: row indices the column sums run over
    (default all; the ``colsum_clamped_row`` mutant passes a list with a repeated last row)."""
    dy, xh = dy.to(dt), xh.to(dt)
    dxh = dy * nw.to(dt)
    m1 = dxh.mean(dim=1, keepdim=True)
    m2 = (dxh * xh).mean(dim=1, keepdim=True)
    ds = r.to(dt)[:, None] * (dxh - m1 - xh * m2)
    du = ds * gelu_grad(pre.to(dt))
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    return dict(ds=ds, du=du, dnw=sel(dy * xh).sum(dim=0), dnb=sel(dy).sum(dim=0), db=sel(du).sum(dim=0),
                ds_abs_colsum=sel(ds.abs()).sum(dim=0))


def backward_stages(dg2, dgb, k, par, wp, bk=None, dt=F64, rounding=True, mutant=None):
    """The fused backward, chained through the bf16 stores ``bk`` = {dugl, du2, du1} (the kernel's own; None:
    this function's own values, rounded when ``rounding``).  k: the forward's stored tensors (g_bf, pre1, xh1,
    r1, vsum, g1_bf, pre2, xh2, r2, g2_bf, pregl).  Returns name -> tensor (``dt``), plus ``_mag_*`` floats: the
    magnitudes the GELU' core error multiplies."""
    B, G = dg2.shape
    K = wp.numel()
    rows = None
    if mutant == "colsum_clamped_row" and B % RB:
        rows = list(range(B)) + [B - 1] * (RB - B % RB)       # the clamped rows >= B of the last tile
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    o = {}
    dy2 = dg2.to(dt)
    if par.get("wgl") is not None:
        o["dugl"] = dgb.to(dt) * gelu_grad(k["pregl"].to(dt))
        o["_mag_dugl"] = float(dgb.abs().max())
        sel = (lambda t: t) if rows is None else (lambda t: t[rows])
        o["dbgl"] = sel(o["dugl"]).sum(dim=0)
        o["_mag_dbgl"] = float(sel(dgb.to(dt).abs()).sum(dim=0).max())
        dugl_s = (bk["dugl"] if bk is not None else store(o["dugl"])).to(dt)
        dy2 = dy2 + dugl_s @ wimg(par["wgl"], dt, rounding)
        o["dWgl"] = dugl_s.t() @ k["g2_bf"].to(dt)
    s2 = st_ln_bwd(dy2, k["xh2"], k["r2"], par["n2w"], k["pre2"], dt, rows)
    o.update(du2=s2["du"], dn2w=s2["dnw"], dn2b=s2["dnb"], db2=s2["db"])
    o["_mag_du2"], o["_mag_db2"] = float(s2["ds"].abs().max()), float(s2["ds_abs_colsum"].max())
    du2_s = (bk["du2"] if bk is not None else store(s2["du"])).to(dt)
    o["dW2"] = du2_s.t() @ k["g1_bf"].to(dt)
    dy1 = s2["ds"] + du2_s @ wimg(par["w2"], dt, rounding)
    s1 = st_ln_bwd(dy1, k["xh1"], k["r1"], par["n1w"], k["pre1"], dt, rows)
    o.update(du1=s1["du"], dn1w=s1["dnw"], dn1b=s1["dnb"], db1=s1["db"])
    o["_mag_du1"], o["_mag_db1"] = float(s1["ds"].abs().max()), float(s1["ds_abs_colsum"].max())
    du1_s = (bk["du1"] if bk is not None else store(s1["du"])).to(dt)
    o["dW1"] = du1_s.t() @ k["g_bf"].to(dt)
    o["dg"] = s1["ds"] + du1_s @ wimg(par["w1"], dt, rounding)
    o["dvs"] = wp.to(dt).mean() * s1["ds"]
    tot = (s1["ds"] * k["vsum"].to(dt)).sum()
    o["dwp"] = (tot if mutant == "dwp_no_k" else tot / K).expand(K).clone()
    o["_stores"] = dict(du2=du2_s, du1=du1_s, **({"dugl": dugl_s} if par.get("wgl") is not None else {}))
    return o


# ---- the general path (glob.hip) ----------------------------------------------------------------------
def row_ln_fwd(u, bias, res, vpart, wp, nw, nb, eps, dt=F64):
    """pbx_row_ln_fwd: z = res + GELU(u + b) [+ mean(wp) sum_t vpart] -> LayerNorm.  One stage with u given."""
    pre = u.to(dt) + bias.to(dt)
    z = res.to(dt) + gelu(pre)
    o = {}
    if vpart is not None:
        o["vsum"] = st_vsum(vpart, dt)
        z = z + wp.to(dt).mean() * o["vsum"]
    m, o["rstd"] = st_row_stats(z, eps, dt)
    o["xhat"], o["out"] = st_ln(z, m, o["rstd"], nw, nb, dt)
    o["_mag"] = float(pre.abs().max())
    return o


def row_ln_bwd(dout, xhat, rstd, gamma, u, bias, vsum=None, wp=None, dt=F64):
    """pbx_row_ln_bwd: one stage of the backward with u given (dres = ds)."""
    s = st_ln_bwd(dout, xhat, rstd, gamma, u.to(dt) + bias.to(dt), dt)
    o = dict(dres=s["ds"], du=s["du"], dgamma=s["dnw"], dbeta=s["dnb"], dbias=s["db"],
             _mag_du=float(s["ds"].abs().max()), _mag_dbias=float(s["ds_abs_colsum"].max()))
    if vsum is not None:
        K = wp.numel()
        o["dvs"] = wp.to(dt).mean() * s["ds"]
        o["dwp"] = ((s["ds"] * vsum.to(dt)).sum() / K).expand(K).clone()
    return o


def bias_gelu(u, bias, dt=F64):
    return gelu(u.to(dt) + bias.to(dt))


def bias_gelu_bwd(dout, u, bias, dt=F64):
    du = dout.to(dt) * gelu_grad(u.to(dt) + bias.to(dt))
    return dict(du=du, dbias=du.sum(dim=0), _mag_du=float(dout.abs().max()),
                _mag_dbias=float(dout.to(dt).abs().sum(dim=0).max()))


# ---- playing the kernel ---------------------------------------------------------------------------------
def play_forward(inp, par, eps, dt=F32, rounding=True, mutant=None):
    """The forward chained on its own outputs; returns the ``k`` dictionary a kernel would have stored."""
    G = inp["g"].shape[1]
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    k = {}
    k["vsum"] = st_vsum(inp["vpart"], dt)
    k["pre1"] = st_pre(inp["g_bf"], par["w1"], par["b1"], dt, rounding)
    k["z1"] = st_z1(inp["g"], k["pre1"], k["vsum"], inp["wp"], dt)
    k["part1"] = st_part(k["z1"], dt)
    m1, k["r1"] = st_merge(k["part1"], G, eps, dt, mutant)
    k["xh1"], o1 = st_ln(k["z1"], m1, k["r1"], par["n1w"], par["n1b"], dt)
    k["g1_bf"] = store(o1)
    k["pre2"] = st_pre(k["g1_bf"], par["w2"], par["b2"], dt, rounding)
    k["z2"] = st_z2(k["g1_bf"] if mutant == "residual_bf16" else o1, k["pre2"], dt)
    k["part2"] = st_part(k["z2"], dt)
    m2, k["r2"] = st_merge(k["part2"], G, eps, dt, mutant)
    k["xh2"], k["g2"] = st_ln(k["z2"], m2, k["r2"], par["n2w"], par["n2b"], dt)
    k["g2_bf"] = store(k["g2"])
    if par.get("wgl") is not None:
        k["pregl"] = st_pre(k["g2_bf"], par["wgl"], par["bgl"], dt, rounding)
        k["gb"] = gelu(k["pregl"])
    k["g_bf"] = inp["g_bf"]
    return k


def play_backward(dg2, dgb, k, par, wp, dt=F32, rounding=True, mutant=None):
    """The backward chained on its own bf16 stores; returns (outputs, stores) as a kernel would leave them."""
    o = backward_stages(dg2, dgb, k, par, wp, None, dt, rounding, mutant)
    stores = o.pop("_stores")
    return o, ({n: v.to(BF16) for n, v in stores.items()} if rounding else stores)


# ---- the comparison helper ----------------------------------------------------------------------------
class Ledger:
    """Collects err / e32 of every checked tensor: ``rows`` in order, ``worst`` the largest ratio by name."""

    def __init__(self):
        self.rows = []
        self.worst = {}

    def add(self, name, err, e32, bound):
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        self.rows.append((name, err, e32, ratio, bound))
        self.worst[name] = max(self.worst.get(name, 0.0), ratio)
        print(f"  {name:<14s} err {err:.3e}  e32 {e32:.3e}  err/e32 {ratio:7.2f}  bound {bound:.3e}")
        return ratio


def check(name, xk, x64, x32, gelu_mag=0.0, ledger=None, e32=None):
    """fp32 store: max |X_k - X_64| <= 16 * max |X_32 - X_64| + 1.5e-7 * gelu_mag.  Returns e32; with ``e32``
    given (and ``x32`` None) that yardstick is used: two kernel forms of one output compared with each other."""
    assert xk.shape == x64.shape and (x32 is None or x32.shape == x64.shape), (name, xk.shape, x64.shape)
    xk = xk.detach().cpu().to(F64)
    x64 = x64.detach().cpu().to(F64)
    assert torch.isfinite(xk).all(), f"{name}: non-finite values stored"
    err = float((xk - x64).abs().max()) if xk.numel() else 0.0
    if x32 is not None:
        e32 = float((x32.detach().cpu().to(F64) - x64).abs().max()) if xk.numel() else 0.0
    bound = MARGIN * e32 + GELU_CORE * gelu_mag
    if ledger is not None:
        ledger.add(name, err, e32, bound)
    assert err <= bound, f"{name}: err {err:.3e} > 16 * {e32:.3e} + {GELU_CORE * gelu_mag:.3e}"
    return e32


def check_bf16(name, xk_bf, x64, x32, gelu_mag=0.0, ledger=None):
    """bf16 store: |X_k - X_64| <= half a bf16 ulp of X_64 + 16 * e32 + gelu_term, elementwise (e32 of the value
    before rounding).  The ledger gets the excess over the half ulp, in units of e32."""
    assert xk_bf.dtype == BF16 and xk_bf.shape == x64.shape == x32.shape, (name, xk_bf.dtype, xk_bf.shape)
    xk = xk_bf.detach().cpu().to(F64)
    x64 = x64.detach().cpu().to(F64)
    assert torch.isfinite(xk).all(), f"{name}: non-finite values stored"
    e32 = float((x32.detach().cpu().to(F64) - x64).abs().max()) if xk.numel() else 0.0
    slack = MARGIN * e32 + GELU_CORE * gelu_mag
    excess = (xk - x64).abs() - bf16_half_ulp(x64)
    worst = max(float(excess.max()), 0.0) if xk.numel() else 0.0
    if ledger is not None:
        ledger.add(name + "(bf16)", worst, e32, slack)
    assert worst <= slack, f"{name}: {worst:.3e} beyond the bf16 half ulp > 16 * {e32:.3e} + {GELU_CORE * gelu_mag:.3e}"


FWD_GELU_MAG = {"z1": "pre1", "z2": "pre2", "gb": "pregl"}     # output -> the stored tensor the cdf multiplies


def check_forward(inp, par, k, eps, ledger=None):
    """Every stored tensor of the fused forward, stage by stage, plus the direct statistics check."""
    o64 = forward_stages(inp, par, k, eps, F64)
    o32 = forward_stages(inp, par, k, eps, F32)
    ngl = par.get("wgl") is not None
    for n in ["vsum", "pre1", "z1", "r1", "xh1", "pre2", "z2", "r2", "xh2", "g2"] + (["pregl", "gb"] if ngl else []):
        mag = float(k[FWD_GELU_MAG[n]].abs().max()) if n in FWD_GELU_MAG else 0.0
        check(n, k[n], o64[n], o32[n], mag, ledger)
    for s in ("1", "2"):
        check(f"part{s}.mean", k["part" + s][..., 0], o64[f"part{s}_mean"], o32[f"part{s}_mean"], 0.0, ledger)
        check(f"part{s}.M2", k["part" + s][..., 1], o64[f"part{s}_M2"], o32[f"part{s}_M2"], 0.0, ledger)
        # the merged statistics against a plain fp64 mean / variance of the full stored row
        check(f"r{s}|plain", k["r" + s], o64[f"r{s}_plain"], o32[f"r{s}_plain"], 0.0, ledger)
        check(f"xh{s}|plain", k["xh" + s], o64[f"xh{s}_plain"], o32[f"xh{s}_plain"], 0.0, ledger)
    check_bf16("g1_bf", k["g1_bf"], o64["o1"], o32["o1"], 0.0, ledger)
    check_bf16("g2_bf", k["g2_bf"], o64["g2"], o32["g2"], 0.0, ledger)
    assert torch.equal(k["g2_bf"].cpu(), rne_bf16(k["g2"].cpu())), "g2_bf is not the RNE bf16 of the stored g2"


BWD_SUMS = ("db1", "dn1w", "dn1b", "db2", "dn2w", "dn2b", "dbgl", "dwp")


def check_backward(dg2, dgb, k, par, wp, got, ledger=None, names=None, pre=None):
    """got: name -> kernel tensor (dugl / du2 / du1 bf16; dg, dvs, the column sums, dW* fp32).  ``pre``: what
    the accumulated destinations held before the launch (added to the oracle).  Returns (fp64 outputs, name -> e32
    of the fp32-stored outputs)."""
    bk = {n: got[n] for n in ("dugl", "du2", "du1") if got.get(n) is not None}
    o64 = backward_stages(dg2, dgb, k, par, wp, bk, F64)
    o32 = backward_stages(dg2, dgb, k, par, wp, bk, F32)
    e32s = {}
    for n in names or [x for x in got if got[x] is not None and not x.startswith("_")]:
        mag = o64.get("_mag_" + n, 0.0)
        if n in ("dugl", "du2", "du1"):
            check_bf16(n, got[n], o64[n], o32[n], mag, ledger)
            continue
        add = 0.0 if pre is None or pre.get(n) is None else pre[n].detach().cpu()
        e32s[n] = check(n, got[n], o64[n].cpu() + (add.to(F64) if torch.is_tensor(add) else 0.0),
                        (o32[n].cpu() + add) if torch.is_tensor(add) else o32[n], mag, ledger)
    return o64, e32s
