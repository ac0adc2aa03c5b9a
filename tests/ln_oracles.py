"""Stage-wise oracles (torch only, float64 by default) for the position-major LayerNorm / local-MLP kernels of
``ops/csrc/ln.hip``: ``pbx_ln_linear_fwd``, ``ln2_consts_kernel`` + ``pbx_ln2_linear_bwd``, ``pbx_embed_fwd`` and
``pbx_embed_bwd`` (``pbx_ln1_finalize`` / ``pbx_embed_dpre`` have theirs in tests/conv_oracles.py).

As in tests/global_oracles.py and tests/conv_oracles.py every stage is evaluated on its own from the tensors the
kernel was given or itself stored for the stage before, once in fp64 (the oracle X_64) and once in plain fp32 torch
ops (the yardstick X_32): ``e32 = max |X_32 - X_64|`` and the fp32 slack of a stage is ``MARGIN * e32``.  No tolerance
is a constant.

* bf16 store: half a bf16 ulp of the fp64 value plus the slack, per element.
* GELU / GELU': the loaded build's form in both precisions; the exact build adds ``GELU_CORE`` times the magnitude
  the core multiplies.
* Hidden roundings.  The forward rounds h1 to bf16 only as the MFMA operand (the residual and the GELU take the fp32
  h1 and pre); the backward does the same with ``dpre = bf16(ds2 GELU'(pre_l))`` and ``bf16(h1)``.  Each gets the
  admissible interval ``[lo, hi]`` of :func:`conv_oracles.interval`; the stages behind it are evaluated at ``lo`` and
  their tolerance gains the drift ``gap @ |W|`` (times the Lipschitz constant of a GELU behind it).  Three conditions
  keep the intervals from hiding a wrong kernel and are asserted on every case: the ambiguous share of the hidden h1
  stays under :data:`AMBIGUOUS_MAX`, that of the hidden dpre under :data:`AMBIGUOUS_DPRE_MAX` (GELU' leaves many
  values near zero, where one absolute slack spans several bf16 values), and the largest drift of a tensor under
  :data:`DRIFT_MAX` of the rms of its fp64 value.
* Every backward stage behind the constants takes the kernel's STORED ``consts``; ``sums1`` / ``dg1`` / ``db1`` take
  the kernel's stored dh1 (it re-reads the packed values), so they carry no drift.
* The six per-sample constants and the tile means of st2 are tensors of few elements (B, B x tiles): the measured
  e32 of one of them can be 0 by luck -- at (L = 33, B = 1) torch's fp32 sums of both tiles are exact and their means
  equal the fp64 ones bit for bit, while the kernel's order of the same fp32 additions rounds once (7.5e-9) -- so
  their yardstick is floored at half an fp32 ulp of the value (:func:`ulp_floor`, 2^-24 max |x|), the precision of
  the format.  tests/test_ln_oracles.py shows the counter-example on the CPU.

:func:`play_forward` / :func:`play_backward` chain the stages on their own outputs.  With ``rounding=False`` in fp64
they are the plain expression (validated against autograd in tests/test_ln_oracles.py); in fp32 with the roundings
on they are a stand-in kernel (the Chan merge of ``wave_ln_stats`` lane by lane, every other sum in the opposite
order to the yardstick's), and with a ``mutant`` name a deliberately wrong one that the checks must reject.
"""
import torch

import conv_oracles as co
from conv_oracles import (ConvLedger, check_bits, check_elem, check_member, check_share, core_term, gelu_pair,  # noqa: F401
                          interval, lipschitz, partial_counts, st_stats)
from global_oracles import BF16, F32, F64, GELU_CORE, MARGIN, Ledger, bf16_half_ulp, rne_bf16, trunc_bf16  # noqa: F401

C = 128                       # channels
PB = 32                       # positions per (mean, M2) partial of s2 (BML of ln.hip)
V = 26                        # vocabulary
EPS = 1e-5                    # local_track.LN_EPS
AMBIGUOUS_MAX = co.AMBIGUOUS_MAX      # hidden h1 (check_share's cap)
AMBIGUOUS_DPRE_MAX = 0.20             # hidden dpre
DRIFT_MAX = 0.02                      # largest drift of a tensor / rms of its fp64 value
WL_SCALE = 0.5                        # of randn / sqrt(C): |pre| stays under ~3 (see make_case)
CONSTS = ("mean2", "rstd2", "m1", "m2", "mean1", "rstd1")
GRADS = ("dg2", "db2", "dg1", "db1", "dwl", "dbl")

MUTANTS = ("m2_term_dropped", "m1_term_dropped", "merge_no_between", "count_full_tile", "bf16_truncate",
           "residual_bf16", "gelu_on_rounded_pre", "chunk_tail_leaks", "odd_tail_row_live", "dwl_reset_per_pair",
           "sums1_from_unrounded_dh1", "consts_slots_swapped")

_e32, _fail = co._e32, co._fail


def _bc(v):
    return v[:, None, None]


def _rms(x):
    return float(x.to(F64).pow(2).mean().sqrt())


def ulp_floor(x64):
    """Half an fp32 ulp of the largest value, 2^-24 max |x|: the floor of the yardstick of a tensor of few elements."""
    return float(x64.abs().max()) * 2.0 ** -24 if x64.numel() else 0.0


# ---- the launchers' grids ------------------------------------------------------------------------------
def fwd_groups(B, L, cus):
    """ln_groups of ln.hip: sample groups of the forward's grid."""
    tp = (L + PB - 1) // PB
    return max(1, min((2 * cus + tp - 1) // tp, B))


def fwd_walks(B, L, cus):
    """The numbers of samples the forward's workgroups walk."""
    g = fwd_groups(B, L, cus)
    return sorted({B * (y + 1) // g - B * y // g for y in range(g)})


def bwd_grid(B, L, det, cus):
    """ln2_bwd_grid of ln.hip: (workgroups over the position pairs, sample splits)."""
    pairs = (L + 1) // 2
    nsplit = min((cus + pairs - 1) // pairs, (B + 15) // 16)
    if nsplit < 1 or det:
        nsplit = 1
    return min(pairs, cus), nsplit


def bwd_walk(B, L, det, cus):
    """What workgroup (0, 0) of the backward walks: (its position pairs, its 16-sample chunks, the sample splits)."""
    gx, nsplit = bwd_grid(B, L, det, cus)
    return list(range(0, (L + 1) // 2, gx)), (B // nsplit + 15) // 16, nsplit


# ---- test inputs --------------------------------------------------------------------------------------
def tile_partials(x, bm, L, out_dt=F32):
    """[B, ceil(L / bm), 2] (mean, M2) partials of ``bm`` positions x 128 channels, from fp64."""
    m, M2, _ = st_stats(x, L, ("rows", bm), F64)
    return torch.stack([m, M2], dim=-1).to(out_dt)


def plain_xhat(x, eps=EPS):
    v = x.to(F64)
    flat = v.reshape(v.shape[0], -1)
    return (v - _bc(flat.mean(1))) * _bc(torch.rsqrt(flat.var(1, unbiased=False) + eps))


def make_sums2(dh2, s2, g2, L, eps=EPS, out_dt=F32):
    """[B, ceil(L / 32), 2]: fp64 sums of dh2 g2 and dh2 g2 xhat2 over tiles of 32 positions, rounded to ``out_dt``."""
    B = dh2.shape[0]
    T = (L + PB - 1) // PB
    dxh = dh2.to(F64) * g2.to(F64)
    both = torch.zeros((2, B, T * PB, C), dtype=F64)
    both[0, :, :L], both[1, :, :L] = dxh, dxh * plain_xhat(s2, eps)
    return both.reshape(2, B, T, PB * C).sum(-1).permute(1, 2, 0).contiguous().to(out_dt)


def make_case(B, L, bm1=128, seed=None, backward=True, plain=False):
    """Inputs of the forward and (``backward``) the backward, chosen so that every term carries weight: s1 has a
    ramp over the positions (the between-tile term of the LayerNorm-1 merge holds > 10 % of the variance once there
    are several partials), dh2 = randn + 0.5 + 0.5 xhat2 (|m1|, |m2| ~ 0.5), every accumulated destination is
    preloaded.  The backward's s2 / pre_l / st2 are an fp64 forward rounded as the kernel stores them.  Wl is half
    the usual randn / sqrt(C): the fitted GELU' in fp32 loses x (c2 + c3 x^2) ulps of 1 - s, and with |pre| up to 5
    the e32 of the hidden dpre (2.9e-6) made 26 % of its elements ambiguous, over the 20 % condition.
    ``plain``: the inputs of tests/test_hip_ln_inflight.py instead (no ramp, dh2 = randn)."""
    gen = torch.Generator().manual_seed(1000 * B + L + 7 * bm1 if seed is None else seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc  # noqa: E731
    c = dict(B=B, L=L, BM1=bm1)
    s1 = rn(B, L, C, sc=1.3) + 0.2
    if not plain:
        s1 = s1 + torch.linspace(-1.0, 1.0, L)[None, :, None]
    c["s1"] = s1.to(BF16)
    c["g1"], c["be1"], c["g2"] = 1.0 + rn(L, C, sc=0.2), rn(L, C, sc=0.2), 1.0 + rn(L, C, sc=0.2)
    c["wl"] = rn(C, C, sc=(1.0 if plain else WL_SCALE) * C ** -0.5).to(BF16)
    c["bl"] = rn(C, sc=0.1)
    c["st1"] = tile_partials(c["s1"], bm1, L)
    if not backward:
        return c
    h1 = plain_xhat(c["s1"]) * c["g1"].to(F64) + c["be1"].to(F64)
    pre = h1 @ c["wl"].to(F64).t() + c["bl"].to(F64)
    c["pre_l"] = pre.to(BF16)
    c["s2"] = (h1 + gelu_pair(pre, "exact")[0]).to(BF16)
    c["st2"] = tile_partials(c["s2"], PB, L)
    dh2 = rn(B, L, C)
    if not plain:
        dh2 = dh2 + 0.5 + 0.5 * plain_xhat(c["s2"]).to(F32)
    c["dh2"] = dh2.to(BF16)
    c["sums2"] = make_sums2(c["dh2"], c["s2"], c["g2"], L)
    for n in ("dg2", "db2", "dg1", "db1"):
        c[n + "_0"] = rn(L, C)
    c["dwl_0"], c["dbl_0"] = rn(C, C), rn(C)
    return c


def bwd_inputs(c):
    """What pbx_ln2_linear_bwd is given beside the parameters."""
    return {n: c[n] for n in ("dh2", "s2", "pre_l", "st2", "sums2", "st1")}


def make_embed_case(rows, seed=3):
    gen = torch.Generator().manual_seed(seed + rows)
    tok = torch.randint(0, V, (rows,), generator=gen)
    tok[:V] = torch.arange(V)                                 # every token value occurs
    return dict(rows=rows, tok=tok.contiguous(), E=torch.randn(V, C, generator=gen) * 0.7,
                dout=torch.randn(rows, C, generator=gen).to(BF16), dE0=torch.randn(V, C, generator=gen))


# ---- statistics ---------------------------------------------------------------------------------------------
def st_merge(st, BM, L, eps=EPS, dt=F64, mutant=None):
    """(mean, rstd) [B] of the (mean, M2) partials by the count-weighted merge."""
    p = st.to(dt)
    cnt = partial_counts(p.shape[1], BM, L, dt, p.device)
    N = cnt.sum()
    mean = (p[..., 0] * cnt).sum(dim=1) / N
    M2 = p[..., 1].sum(dim=1)
    if mutant != "merge_no_between":
        M2 = M2 + (cnt * (p[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    return mean, torch.rsqrt(M2 / N + eps)


def chan_merge_wave(st, BM, L, eps=EPS, mutant=None):
    """wave_ln_stats of mfma.h in fp32: lane t merges partials t, t + 64, ..., then a butterfly over the 64 lanes."""
    p = st.to(F32)
    B, T = p.shape[0], p.shape[1]
    cnt = partial_counts(T, BM, L, F32, p.device)
    between = 0.0 if mutant == "merge_no_between" else 1.0

    def merge(n, m, M2, nb, mb, M2b):
        nn = n + nb
        f = torch.where(nn > 0, nb / torch.where(nn > 0, nn, torch.ones_like(nn)), torch.zeros_like(nn))
        d = mb - m
        return nn, m + d * f, torch.where(nn > 0, M2 + (M2b + between * d * d * n * f), M2)

    n, m, M2 = (torch.zeros((B, 64), dtype=F32) for _ in range(3))
    for t0 in range(0, T, 64):
        w = min(64, T - t0)
        pad = lambda v: torch.cat([v, torch.zeros((B, 64 - w), dtype=F32)], dim=1)  # noqa: E731
        n, m, M2 = merge(n, m, M2, pad(cnt[t0:t0 + w].expand(B, w)), pad(p[:, t0:t0 + w, 0]), pad(p[:, t0:t0 + w, 1]))
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        n, m, M2 = merge(n, m, M2, n[:, lanes ^ o], m[:, lanes ^ o], M2[:, lanes ^ o])
    return m[:, 0], torch.rsqrt(M2[:, 0] / n[:, 0] + eps)


def st_consts(k, BM1, L, eps=EPS, dt=F64, mutant=None):
    """[B, 6] (mean2, rstd2, m1, m2, mean1, rstd1) from the given st2 (tiles of 32), sums2 and st1."""
    mean2, rstd2 = st_merge(k["st2"], PB, L, eps, dt)
    q = k["sums2"].to(dt)
    mean1, rstd1 = st_merge(k["st1"], BM1, L, eps, dt, mutant)
    return torch.stack([mean2, rstd2, q[..., 0].sum(dim=1) / (L * C), q[..., 1].sum(dim=1) / (L * C), mean1, rstd1], dim=1)


def between_share(st, BM, L):
    """The smallest share over the samples of the between-tile term in the merged M2."""
    p = st.to(F64)
    cnt = partial_counts(p.shape[1], BM, L, F64)
    mean = (p[..., 0] * cnt).sum(dim=1) / cnt.sum()
    btw = (cnt * (p[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    return float((btw / (btw + p[..., 1].sum(dim=1))).min())


# ---- forward -------------------------------------------------------------------------------------------------
def st_h1(c, mean, rstd, dt=F64):
    return (c["s1"].to(dt) - _bc(mean.to(dt))) * _bc(rstd.to(dt)) * c["g1"].to(dt) + c["be1"].to(dt)


def st_pre(hb, c, dt=F64, rev=False):
    w = c["wl"].to(dt)
    if rev:
        return hb.to(dt).flip(-1) @ w.flip(-1).t() + c["bl"].to(dt)
    return hb.to(dt) @ w.t() + c["bl"].to(dt)


def _drift_cond(name, drift, x64, ledger, fails):
    ratio = float(drift.max()) / _rms(x64)
    if ledger is not None:
        ledger.note("drift / rms " + name, ratio)
    if not ratio < DRIFT_MAX:
        _fail(fails, name, f"largest drift {float(drift.max()):.3e} is {ratio:.3f} of the rms, >= {DRIFT_MAX}")


def forward_ref(c, mode, ledger=None, fails=None, tag="fwd"):
    """Everything of :func:`check_forward` that does not depend on the kernel's outputs: the admissible bf16 h1,
    pre_l and s2 in fp64 at its low end, their e32 and free terms, and the conditions on the share and the drifts."""
    L, BM1 = c["L"], c["BM1"]
    lg, _ = lipschitz(mode)
    core = core_term(mode)
    h64 = st_h1(c, *st_merge(c["st1"], BM1, L, dt=F64), F64)
    h32 = st_h1(c, *st_merge(c["st1"], BM1, L, dt=F32), F32)
    e = _e32(h32, h64)
    lo, hi, gap = interval(h64, MARGIN * e)
    if ledger is not None:
        ledger.note(f"e32 {tag}.h1", e)
    check_share(f"{tag}.h1", gap, ledger, fails)
    p64, p32 = st_pre(lo, c, F64), st_pre(lo.to(F32), c, F32)
    drift = gap @ c["wl"].to(F64).abs().t()
    ref = dict(h1=(lo, hi, gap))
    ref["pre_l"] = (p64, _e32(p32, p64), bf16_half_ulp(p64.abs() + drift) + drift)
    _drift_cond(f"{tag}.pre_l", drift, p64, ledger, fails)
    s64 = h64 + gelu_pair(p64, mode)[0]
    s32 = h32 + gelu_pair(p32, mode)[0]
    d2 = lg * drift
    ref["s2"] = (s64, _e32(s32, s64), bf16_half_ulp(s64.abs() + d2) + d2 + core * (p64.abs() + drift))
    _drift_cond(f"{tag}.s2", d2, s64, ledger, fails)
    return ref


def check_stats(s2, st2, L, ledger=None, fails=None, tag="fwd"):
    """The (mean, M2) partials per 32 positions against the stored s2 (the checks of conv_oracles.check_forward)."""
    layout = ("rows", PB)
    m64, M64, sq64 = st_stats(s2, L, layout, F64)
    m32, M32, _ = st_stats(s2.to(F32), L, layout, F32)
    if tuple(st2.shape) != (*m64.shape, 2):
        return _fail(fails, f"{tag}.st2", f"shape {tuple(st2.shape)}, expected {(*m64.shape, 2)}")
    check_elem(f"{tag}.mean", st2[..., 0], m64, max(_e32(m32, m64), ulp_floor(m64)), None, ledger, fails)
    e2p, ulp = _e32(M32, M64), float((2.0 ** -24 * sq64).max())
    errM = float((st2[..., 1].to(F64) - M64).abs().max())
    if ledger is not None:
        ledger.note(f"{tag}.M2 err / (2^-24 sumsq)", errM / ulp)
        ledger.note(f"{tag}.M2 err / two-pass e32", errM / e2p if e2p > 0 else 0.0)
    check_elem(f"{tag}.M2", st2[..., 1], M64, max(e2p, ulp), None, ledger, fails)


def check_forward(c, k, mode, ledger=None, fails=None, tag="fwd", ref=None):
    """k: the kernel's pre_l (None: the inference form), s2 (bf16 [B, L, C]) and st2 [B, ceil(L / 32), 2]."""
    ref = forward_ref(c, mode, ledger, fails, tag) if ref is None else ref
    if k.get("pre_l") is not None:
        check_elem(f"{tag}.pre_l(bf16)", k["pre_l"], *ref["pre_l"], ledger, fails)
    check_elem(f"{tag}.s2(bf16)", k["s2"], *ref["s2"], ledger, fails)
    check_stats(k["s2"], k["st2"], c["L"], ledger, fails, tag)


def play_forward(c, mode, dt=F32, rounding=True, mutant=None, eps=EPS):
    """The forward chained on its own outputs; returns what a kernel would have stored (plus the hidden ``hb``)."""
    L, BM1 = c["L"], c["BM1"]
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    if rounding and dt == F32:
        mean, rstd = chan_merge_wave(c["st1"], BM1, L, eps, mutant)
    else:
        mean, rstd = st_merge(c["st1"], BM1, L, eps, dt, mutant)
    h1 = st_h1(c, mean, rstd, dt)
    hb = rne_bf16(h1).to(dt) if rounding else h1
    pre = st_pre(hb, c, dt, rev=rounding)
    gin = rne_bf16(pre).to(dt) if mutant == "gelu_on_rounded_pre" else pre
    s2 = (hb if mutant == "residual_bf16" else h1) + gelu_pair(gin, mode)[0]
    k = dict(pre_l=store(pre), s2=store(s2), hb=hb)
    m, M2, _ = st_stats(k["s2"].to(dt), L, ("rows", PB), dt, onepass=rounding)
    if mutant == "count_full_tile" and L % PB:                 # sum / (32 x 128) in the partial last tile
        sa = m[:, -1] * ((L % PB) * C)
        sq = M2[:, -1] + sa * m[:, -1]
        mw = sa / (PB * C)
        m = torch.cat([m[:, :-1], mw[:, None]], dim=1)
        M2 = torch.cat([M2[:, :-1], (sq - sa * mw).clamp(min=0)[:, None]], dim=1)
    k["st2"] = torch.stack([m, M2], dim=-1)
    return k


# ---- backward ------------------------------------------------------------------------------------------------
def check_consts(c, k, consts, ledger=None, fails=None, tag="bwd", eps=EPS):
    """The six per-sample constants from the given partials; slots 6 and 7 exactly 0."""
    L = c["L"]
    if tuple(consts.shape) != (c["B"], 8):
        return _fail(fails, f"{tag}.consts", f"shape {tuple(consts.shape)}")
    c64, c32 = st_consts(k, c["BM1"], L, eps, F64), st_consts(k, c["BM1"], L, eps, F32)
    for i, n in enumerate(CONSTS):
        e = max(_e32(c32[:, i], c64[:, i]), ulp_floor(c64[:, i]))
        check_elem(f"{tag}.consts.{n}", consts[:, i], c64[:, i], e, None, ledger, fails)
    if not bool((consts[:, 6:] == 0).all()):
        _fail(fails, f"{tag}.consts.pad", "slots 6 and 7 are not 0")


def _pair_sums(x, L):
    """[B, ceil(L / 2)]: sums over the (up to) two positions of every pair and the channels."""
    B, TS1 = x.shape[0], (L + 1) // 2
    if L % 2:
        x = torch.cat([x, torch.zeros((B, 1, C), dtype=x.dtype)], dim=1)
    return x.reshape(B, TS1, 2 * C).sum(dim=-1)


def backward_ref(c, k, consts, mode, ledger=None, fails=None, tag="bwd"):
    """Everything of :func:`check_backward` that depends on the kernel's outputs through its stored ``consts``
    only (one reference serves every launch mode of a case: their consts are bitwise equal)."""
    _, lgd = lipschitz(mode)
    core = core_term(mode)
    cs = consts.to(F32)

    def stages(dt):
        mean2, rstd2, m1, m2, mean1, rstd1 = (_bc(cs[:, i].to(dt)) for i in range(6))
        dh2 = k["dh2"].to(dt)
        xh2 = (k["s2"].to(dt) - mean2) * rstd2
        o = dict(dg2=c["dg2_0"].to(dt) + (dh2 * xh2).sum(dim=0), db2=c["db2_0"].to(dt) + dh2.sum(dim=0))
        o["ds2"] = rstd2 * (dh2 * c["g2"].to(dt) - m1 - xh2 * m2)
        o["dp"] = o["ds2"] * gelu_pair(k["pre_l"].to(dt), mode)[1]
        o["xh1"] = (c["s1"].to(dt) - mean1) * rstd1
        o["h1"] = o["xh1"] * c["g1"].to(dt) + c["be1"].to(dt)
        return o

    o64, o32 = stages(F64), stages(F32)
    e_dp, e_h = _e32(o32["dp"], o64["dp"]), _e32(o32["h1"], o64["h1"])
    lo_dp, _, gap_dp = interval(o64["dp"], MARGIN * e_dp + core * o64["ds2"].abs())
    lo_h, _, gap_h = interval(o64["h1"], MARGIN * e_h)
    share = float((gap_dp > 0).double().mean())
    if ledger is not None:
        ledger.note(f"e32 {tag}.dpre", e_dp)
        ledger.note(f"e32 {tag}.h1", e_h)
        ledger.note(f"ambiguous {tag}.dpre", share)
    if not share < AMBIGUOUS_DPRE_MAX:
        _fail(fails, f"{tag}.dpre", f"ambiguous share {share:.3f} >= {AMBIGUOUS_DPRE_MAX}")
    check_share(f"{tag}.h1", gap_h, ledger, fails)
    ref = dict(xh1=(o64["xh1"], o32["xh1"]), dpre=(lo_dp, lo_dp + gap_dp), hv=(lo_h, lo_h + gap_h))
    for n in ("dg2", "db2"):
        ref[n] = (o64[n], _e32(o32[n], o64[n]), None)
    w64 = c["wl"].to(F64)
    d64 = o64["ds2"] + lo_dp @ w64
    d32 = o32["ds2"] + lo_dp.to(F32) @ c["wl"].to(F32)
    drift = gap_dp @ w64.abs()
    ref["dh1"] = (d64, _e32(d32, d64), bf16_half_ulp(d64.abs() + drift) + drift)
    _drift_cond(f"{tag}.dh1", drift, d64, ledger, fails)
    b64 = c["dbl_0"].to(F64) + lo_dp.sum(dim=(0, 1))
    b32 = c["dbl_0"] + lo_dp.to(F32).sum(dim=(0, 1))
    drift = gap_dp.sum(dim=(0, 1))
    ref["dbl"] = (b64, _e32(b32, b64), drift)
    _drift_cond(f"{tag}.dbl", drift, b64, ledger, fails)
    dp2, h2, gd2, gh2 = (t.reshape(-1, C) for t in (lo_dp, lo_h, gap_dp, gap_h))
    w_64 = c["dwl_0"].to(F64) + dp2.t() @ h2
    w_32 = c["dwl_0"] + dp2.to(F32).t() @ h2.to(F32)
    drift = gd2.t() @ h2.abs() + dp2.abs().t() @ gh2 + gd2.t() @ gh2
    ref["dwl"] = (w_64, _e32(w_32, w_64), drift)
    _drift_cond(f"{tag}.dwl", drift, w_64, ledger, fails)
    return ref


def check_backward(c, got, ref, ledger=None, fails=None, tag="bwd", names=None):
    """got: dh1 (bf16), sums1 [B, ceil(L / 2), 2] and the six accumulated gradients after the launch."""
    L = c["L"]
    names = names or ("dh1", "sums1", *GRADS)
    for n in ("dh1", "dg2", "db2", "dbl", "dwl"):
        if n in names:
            check_elem(f"{tag}.{n}" + ("(bf16)" if n == "dh1" else ""), got[n], *ref[n], ledger, fails)
    res = []
    for dt, xh in zip((F64, F32), ref["xh1"]):
        d = got["dh1"].to(dt)
        dxh = d * c["g1"].to(dt)
        res.append(dict(sums1=torch.stack([_pair_sums(dxh, L), _pair_sums(dxh * xh, L)], dim=-1),
                        dg1=c["dg1_0"].to(dt) + (d * xh).sum(dim=0), db1=c["db1_0"].to(dt) + d.sum(dim=0)))
    if "sums1" in names:
        if tuple(got["sums1"].shape) != tuple(res[0]["sums1"].shape):
            return _fail(fails, f"{tag}.sums1", f"shape {tuple(got['sums1'].shape)}")
        for i, n in enumerate(("sums1.dxh", "sums1.dxh_xhat")):
            check_elem(f"{tag}.{n}", got["sums1"][..., i], res[0]["sums1"][..., i],
                       _e32(res[1]["sums1"][..., i], res[0]["sums1"][..., i]), None, ledger, fails)
    for n in ("dg1", "db1"):
        if n in names:
            check_elem(f"{tag}.{n}", got[n], res[0][n], _e32(res[1][n], res[0][n]), None, ledger, fails)


def play_backward(c, k, mode, dt=F32, rounding=True, mutant=None, gx=None, eps=EPS):
    """The backward chained on its own outputs.  k: :func:`bwd_inputs`.  ``gx``: workgroups over the position
    pairs (default one per pair; fewer: a workgroup walks pairs x, x + gx, ...)."""
    B, L = c["B"], c["L"]
    TS1 = (L + 1) // 2
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    standin = rounding and dt == F32
    if standin:
        q = k["sums2"].to(F32).flip(1)
        cs = torch.stack([*chan_merge_wave(k["st2"], PB, L, eps), q[..., 0].sum(dim=1) * (1.0 / (L * C)),
                          q[..., 1].sum(dim=1) * (1.0 / (L * C)), *chan_merge_wave(k["st1"], c["BM1"], L, eps, mutant)],
                         dim=1)
    else:
        cs = st_consts(k, c["BM1"], L, eps, dt, mutant)
    if mutant == "consts_slots_swapped":
        cs = cs[:, [0, 1, 3, 2, 4, 5]]
    got = dict(consts=torch.cat([cs, torch.zeros((B, 2), dtype=cs.dtype)], dim=1))
    mean2, rstd2, m1, m2, mean1, rstd1 = (_bc(cs[:, i]) for i in range(6))
    order = (lambda t: t.flip(0)) if standin else (lambda t: t)       # the samples summed in the other order
    dh2, g1 = k["dh2"].to(dt), c["g1"].to(dt)
    xh2 = (k["s2"].to(dt) - mean2) * rstd2
    tail = (-B) % 16 if mutant == "chunk_tail_leaks" else 0            # the clamped sample B - 1, counted again
    got["dg2"] = c["dg2_0"].to(dt) + order(dh2 * xh2).sum(dim=0) + tail * (dh2[-1] * xh2[-1])
    got["db2"] = c["db2_0"].to(dt) + order(dh2).sum(dim=0) + tail * dh2[-1]
    ds2 = dh2 * c["g2"].to(dt)
    if mutant != "m1_term_dropped":
        ds2 = ds2 - m1
    if mutant != "m2_term_dropped":
        ds2 = ds2 - xh2 * m2
    ds2 = rstd2 * ds2
    dp = ds2 * gelu_pair(k["pre_l"].to(dt), mode)[1]
    xh1 = (c["s1"].to(dt) - mean1) * rstd1
    h1 = xh1 * g1 + c["be1"].to(dt)
    if rounding:
        dp, h1 = rne_bf16(dp).to(dt), rne_bf16(h1).to(dt)
    got["_dpre"], got["_hv"] = dp, h1
    w = c["wl"].to(dt)
    dh1 = ds2 + (dp.flip(-1) @ w.flip(0) if standin else dp @ w)
    got["dh1"] = store(dh1)
    d = dh1 if mutant == "sums1_from_unrounded_dh1" else got["dh1"].to(dt)
    dxh = d * g1
    sa, sc = _pair_sums(dxh, L), _pair_sums(dxh * xh1, L)
    if mutant == "odd_tail_row_live" and L % 2:                        # the row past L reads the clamped row L - 1
        sa[:, -1] += dxh[:, -1].sum(dim=-1)
        sc[:, -1] += (dxh * xh1)[:, -1].sum(dim=-1)
    got["sums1"] = torch.stack([sa, sc], dim=-1)
    d = got["dh1"].to(dt)
    got["dg1"] = c["dg1_0"].to(dt) + order(d * xh1).sum(dim=0)
    got["db1"] = c["db1_0"].to(dt) + order(d).sum(dim=0)
    got["dbl"] = c["dbl_0"].to(dt) + order(dp).sum(dim=(0, 1))
    dpw = dp
    if mutant == "dwl_reset_per_pair" and gx is not None and gx < TS1:    # only the last pair of a walk survives
        live = (torch.arange(L) // 2 >= TS1 - gx).to(dt)
        dpw = dp * live[None, :, None]
    got["dwl"] = c["dwl_0"].to(dt) + order(dpw).reshape(-1, C).t() @ order(h1).reshape(-1, C)
    return got


# ---- embedding -----------------------------------------------------------------------------------------------
def check_embed_fwd(e, out, fails=None, tag="embed_fwd"):
    """pbx_embed_fwd: bitwise the RNE bf16 of the looked-up rows."""
    check_bits(f"{tag}.out", out, rne_bf16(e["E"][e["tok"]]), fails)


def check_embed_bwd(e, dE, ledger=None, fails=None, tag="embed_bwd"):
    """pbx_embed_bwd: dE - dE0 = index_add of dout over the tokens."""
    e64 = e["dE0"].to(F64).index_add(0, e["tok"], e["dout"].to(F64))
    e32 = e["dE0"].index_add(0, e["tok"], e["dout"].to(F32))
    check_elem(f"{tag}.dE", dE, e64, _e32(e32, e64), None, ledger, fails)
