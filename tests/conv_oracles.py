"""Stage-wise oracles (torch only, float64 by default) for the local track's dual-dilation conv kernels: the
forwards of ``ops/csrc/conv2.hip`` / ``conv5.hip`` / ``conv_tok.hip``, the data gradient of ``ops/csrc/conv4.hip``
(plain and with the LayerNorm-1 finalize fused in) and ``pbx_ln1_finalize`` / ``pbx_embed_dpre`` of ``ops/csrc/ln.hip``.

As in tests/global_oracles.py every stage is evaluated on its own from the tensors the kernel itself stored or was
given for the stage before, once in fp64 (the oracle X_64) and once in plain fp32 torch ops (the yardstick X_32):
``e32 = max |X_32 - X_64|`` and the fp32 slack of a stage is ``MARGIN * e32``.  No tolerance is a constant.

* bf16 store: half a bf16 ulp of the fp64 value plus the slack, per element (:func:`check_elem`).
* GELU / GELU': the loaded build's form in fp64 (:func:`gelu_pair`; the fitted logistic constants of ``common.h``
  or the erf form).  The exact build adds ``GELU_CORE`` (the A&S 7.1.26 bound) times the magnitude it multiplies;
  for the fitted build the yardstick is the same formula in fp32.
* Hidden roundings.  The forward rounds ``pre + bias`` to bf16 and never stores it, ``pbx_conv_dgrad4f`` does the
  same with dS1.  :func:`interval` gives the admissible interval ``[lo, hi] = [RNE(v64 - slack), RNE(v64 + slack)]``
  (``gap = hi - lo`` is 0 for most elements); a stored value must lie in it (membership, not equality with an end:
  near zero the interval holds more than two bf16 values), downstream stages are evaluated at ``lo`` and their
  tolerance gains ``Lip * gap``, ``Lip`` being 1.01 x the Lipschitz constant of the downstream fp64 function
  (:func:`lipschitz`; ``|gd|`` for a product with ``gd``).  The half ulp of such a downstream value is taken at
  ``|v64| + Lip * gap``, the largest magnitude the admissible values reach: a value evaluated at ``hi`` may sit in
  the next binade.  The share of elements with ``gap > 0`` must stay under :data:`AMBIGUOUS_MAX` per tensor.
* Products of two bf16 values are exact in fp32: ``dpre = bf16(ds1 * gd)`` is asserted bitwise.

:func:`play_forward` / :func:`play_backward` chain the stages on their own outputs.  With ``rounding=False`` in
fp64 they are the plain block expression (validated against autograd in tests/test_conv_oracles.py); in fp32 with
the roundings on they are a stand-in kernel (its taps summed in the opposite order to the yardstick's), and with a
``mutant`` name a deliberately wrong one that the checks must reject.
"""
import functools
import math

import torch

from global_oracles import BF16, F32, F64, GELU_CORE, MARGIN, Ledger, bf16_half_ulp, rne_bf16, trunc_bf16

C = 128                  # channels
KS = 9                   # taps
DIL = 5                  # dilation of the wide conv
BM = 128                 # positions per conv tile (= one LayerNorm-1 partial of conv_fwd3 / conv_fwd5)
V = 26                   # vocabulary of the token form
EPS = 1e-5               # local_track.LN_EPS
AMBIGUOUS_MAX = 0.10     # admissible share of elements whose hidden rounding is not determined
FIT = (-0.10053117, -2.3073633, 1.59934236, 0.20904868)     # the fitted logistic core of common.h
FIT_CLAIM = (2.9e-4, 7.8e-4)   # max |err| common.h states for it in GELU / GELU' against the erf GELU on [-14, 14]

MUTANTS = ("drop_edge_tap", "clamp_pad", "bf16_truncate", "pre_not_rounded", "halo_off_by_one", "dgrad_shift_sign",
           "chan_count_full_tile", "m2_dropped", "fma_contracted_sum")


class ConvLedger(Ledger):
    """The global ledger plus ``notes``: name -> largest value of the ambiguous shares and the M2 ratios."""

    def __init__(self):
        super().__init__()
        self.notes = {}

    def note(self, name, value):
        self.notes[name] = max(self.notes.get(name, 0.0), float(value))
        print(f"  {name:<26s} {float(value):.4g}")


# ---- GELU forms ---------------------------------------------------------------------------------------
def gelu_parts(x, mode):
    """(s, GELU') of the build ``mode`` ("fitted" | "exact") in the dtype of ``x``; GELU = x s."""
    if mode == "exact":
        Phi = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
        phi = torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))
        return Phi, Phi + x * phi
    assert mode == "fitted", mode
    t = x * x
    s = 1.0 / (1.0 + torch.exp2((t * FIT[0] + FIT[1]) * x))
    return s, s + x * s * (1.0 - s) * (FIT[2] + FIT[3] * t)


def gelu_pair(x, mode):
    """(GELU, GELU') of the build."""
    s, gd = gelu_parts(x, mode)
    return x * s, gd


def grid64(n=(1 << 20) + 1):
    return torch.linspace(-14.0, 14.0, n, dtype=F64)


@functools.lru_cache(maxsize=None)
def lipschitz(mode):
    """1.01 x the Lipschitz constants of (GELU, GELU') of the build on [-14, 14]: the largest slope between
    neighbours of a 2^20-point fp64 grid (the slope of a chord never exceeds the supremum of the derivative, and
    with |f''| <= 2 it is within 3e-5 of it at this spacing: 1.01 covers that)."""
    x = grid64()
    h = float(x[1] - x[0])
    g, gd = gelu_pair(x, mode)
    return 1.01 * float((g[1:] - g[:-1]).abs().max()) / h, 1.01 * float((gd[1:] - gd[:-1]).abs().max()) / h


def core_term(mode):
    """What the erf core of the exact build may add per unit of the magnitude it multiplies."""
    return GELU_CORE if mode == "exact" else 0.0


# ---- test inputs --------------------------------------------------------------------------------------
def make_case(B, L, lo=0, hi=0, gb_shift=0.0, tok=False, seed=None, dev="cpu"):
    """Inputs at the scales of tests/test_hip_conv_fwd5.py.  ``lo`` / ``hi``: neighbour rows around each sample
    (x, ds1 and the synthetic GELU' images are [B, lo + L + hi, C]).  ``tok``: x = emb[tok] (the first block)."""
    gen = torch.Generator().manual_seed(1000 * B + L + 7 * lo if seed is None else seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc  # noqa: E731
    R = lo + L + hi
    c = dict(B=B, L=L, lo=lo, hi=hi)
    if tok:
        assert lo == hi == 0
        c["emb"] = rn(V, C, sc=0.7).to(BF16)
        t = torch.randint(0, V, (B, L), generator=gen)
        t[0, :V] = torch.arange(V)                         # every token value occurs
        c["tok"] = t.contiguous()
        c["x"] = c["emb"][c["tok"]]
    else:
        c["x"] = rn(B, R, C, sc=0.7).to(BF16)
    c["wn"], c["ww"] = rn(C, C, KS, sc=0.04), rn(C, C, KS, sc=0.04)
    c["bn"], c["bw"] = rn(C, sc=0.1), rn(C, sc=0.1)
    c["gb"] = rn(B, C, sc=0.5) + gb_shift
    # backward
    c["dh1"] = rn(B, L, C).to(BF16)
    c["g1"] = 1.0 + rn(L, C, sc=0.1)
    c["ds1"] = rn(B, R, C).to(BF16)
    c["gdn"] = (torch.rand(B, R, C, generator=gen) * 1.25 - 0.125).to(BF16)      # the range of a GELU'
    c["gdw"] = (torch.rand(B, R, C, generator=gen) * 1.25 - 0.125).to(BF16)
    c["dgb0"] = rn(B, C)
    c["dE0"] = rn(V, C)
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}


# ---- the convolution as a sum of nine shifted products -----------------------------------------------------
def gather(src, d, L, lo, hi, mutant=None):
    """[B, L + 8 d, C]: logical positions -4 d .. L + 4 d - 1 of ``src`` (its row 0 is position -lo), zero outside
    [-lo, L + hi)."""
    B, H = src.shape[0], 4 * d
    out = torch.zeros((B, L + 2 * H, src.shape[2]), dtype=src.dtype, device=src.device)
    a, b = max(-lo, -H), min(L + hi, L + H)
    out[:, a + H:b + H] = src[:, a + lo:b + lo]
    if mutant == "clamp_pad":
        out[:, :a + H] = src[:, a + lo:a + lo + 1]
        out[:, b + H:] = src[:, b + lo - 1:b + lo]
    if mutant == "halo_off_by_one" and a < 0:             # positions < 0 read one row late
        out[:, a + H:H] = src[:, a + lo + 1:lo + 1]
    return out


def conv_sum(src, w, d, L, lo, hi, dt, sign=1, rounding=True, mutant=None, rev=False):
    """out[pos] = sum_k src[pos + sign (k - 4) d] @ M_k with M_k = bf16(W[:, :, k])^T (sign +1, the forward:
    W is [co, ci, k]) or bf16(W[:, :, k]) (sign -1, the data gradient).  ``rev``: taps summed 8 .. 0."""
    g = gather(src.to(dt), d, L, lo, hi, mutant)
    wd = (rne_bf16(w) if rounding else w).to(dt)
    H = 4 * d
    out = None
    for k in (range(KS - 1, -1, -1) if rev else range(KS)):
        s = H + sign * (k - KS // 2) * d
        term = g[:, s:s + L] @ (wd[:, :, k].t() if sign > 0 else wd[:, :, k])
        if mutant == "drop_edge_tap" and k == 0 and d == DIL and sign > 0:
            term[:, L - 1] = 0
        out = term if out is None else out + term
    return out


def x_mid(c):
    return c["x"][:, c["lo"]:c["lo"] + c["L"]]


def st_pre(c, dt=F64, rounding=True, mutant=None, rev=False):
    """(pre_n, pre_w) = conv + bias, before the hidden rounding."""
    a = (c["L"], c["lo"], c["hi"], dt, 1, rounding, mutant, rev)
    return (conv_sum(c["x"], c["wn"], 1, *a) + c["bn"].to(dt), conv_sum(c["x"], c["ww"], DIL, *a) + c["bw"].to(dt))


def st_out(c, pn, pw, mode, dt=F64, mutant=None):
    """(GELU'(pre_n), GELU'(pre_w), ((x + G(pre_n)) + G(pre_w)) + gb) from the (rounded) pre-activations."""
    gn, dn = gelu_pair(pn.to(dt), mode)
    gw, dw = gelu_pair(pw.to(dt), mode)
    x = x_mid(c).to(dt)
    if mutant == "fma_contracted_sum" and dt == F32:       # x + pre_n * s as one fma: the product is not rounded
        first = (x.to(F64) + pn.to(F64) * gelu_parts(pn.to(dt), mode)[0].to(F64)).to(F32)
    else:
        first = x + gn
    return dn, dw, (first + gw) + c["gb"].to(dt)[:, None, :]


# ---- LayerNorm-1 partials -----------------------------------------------------------------------------------
def tiles_of(s1, L, layout):
    """The values every partial counts: (vals [B, P, N] zero-padded, cnt [P], mask [P, N]).  layout ("rows", bm):
    partial t = rows t bm .. of all 128 channels; ("tok",): conv_fwd_tok's [tile][half 2][wave 16] partials of
    8 positions x 64 channels."""
    B = s1.shape[0]
    if layout[0] == "tok":
        T = L // BM
        v = s1.reshape(B, T, 16, 8, 2, 64).permute(0, 1, 4, 2, 3, 5).reshape(B, T * 32, 512)
        return v, torch.full((T * 32,), 512.0, dtype=F64, device=s1.device), None
    bm = layout[1]
    T = (L + bm - 1) // bm
    v = torch.zeros((B, T * bm, C), dtype=s1.dtype, device=s1.device)
    v[:, :L] = s1
    rows = torch.clamp(L - torch.arange(T, device=s1.device) * bm, max=bm)
    mask = (torch.arange(bm, device=s1.device)[None, :] < rows[:, None]).repeat_interleave(C, dim=1)
    return v.reshape(B, T, bm * C), (rows * C).to(F64), mask


def st_stats(s1, L, layout, dt=F64, onepass=False):
    """(mean, M2, sum of squares) [B, P] of the stored s1.  ``onepass``: sumsq - sum * mean (what the kernels do)."""
    v, cnt, mask = tiles_of(s1, L, layout)
    v, cnt = v.to(dt), cnt.to(dt)
    sa, sq = v.sum(dim=-1), (v * v).sum(dim=-1)
    m = sa / cnt
    if onepass:
        return m, torch.clamp(sq - sa * m, min=0), sq
    d = v - m[..., None]
    if mask is not None:
        d = d * mask.to(dt)
    return m, (d * d).sum(dim=-1), sq


def partial_counts(T1, BM1, L, dt=F64, dev="cpu", mutant=None):
    rows = torch.clamp(L - torch.arange(T1, device=dev) * BM1, max=BM1)
    if mutant == "chan_count_full_tile":
        rows = torch.full_like(rows, BM1)
    return (rows * C).to(dt)


def st_ln1_consts(st1, BM1, sums1, L, eps=EPS, dt=F64, mutant=None):
    """(mean1, rstd1, m1, m2) [B]: the Chan merge of the (mean, M2) partials and the sums of the backward partials."""
    p, q = st1.to(dt), sums1.to(dt)
    cnt = partial_counts(p.shape[1], BM1, L, dt, p.device, mutant)
    N = cnt.sum()
    mean = (p[..., 0] * cnt).sum(dim=1) / N
    M2 = p[..., 1].sum(dim=1) + (cnt * (p[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    m1, m2 = q[..., 0].sum(dim=1) / (L * C), q[..., 1].sum(dim=1) / (L * C)
    if mutant == "m2_dropped":
        m2 = torch.zeros_like(m2)
    return mean, torch.rsqrt(M2 / N + eps), m1, m2


def st_ds1(dh1, s1, g1, consts, dt=F64):
    mean, rstd, m1, m2 = (t.to(dt)[:, None, None] for t in consts)
    return rstd * (dh1.to(dt) * g1.to(dt) - m1 - (s1.to(dt) - mean) * rstd * m2)


def make_sums1(dh1, s1, g1, st1, BM1, L, TS1, eps=EPS, out_dt=F32):
    """[B, TS1, 2] backward partials (rounded to fp32): fp64 sums of dh1 g1 and dh1 g1 xhat1 over (position, 32-channel block)
    pieces, piece i added to entry i mod TS1 (every entry takes part when TS1 <= 4 L)."""
    B = dh1.shape[0]
    cnt = partial_counts(st1.shape[1], BM1, L, F64, st1.device)
    p = st1.to(F64)
    mean = (p[..., 0] * cnt).sum(dim=1) / cnt.sum()
    M2 = p[..., 1].sum(dim=1) + (cnt * (p[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    rstd = torch.rsqrt(M2 / cnt.sum() + eps)
    dxh = dh1.to(F64) * g1.to(F64)
    xh = (s1.to(F64) - mean[:, None, None]) * rstd[:, None, None]
    pieces = torch.stack([dxh.reshape(B, L * 4, 32).sum(-1), (dxh * xh).reshape(B, L * 4, 32).sum(-1)], dim=-1)
    out = torch.zeros((B, TS1, 2), dtype=F64, device=dh1.device)
    out.index_add_(1, torch.arange(L * 4, device=dh1.device) % TS1, pieces)
    return out.to(out_dt)


# ---- the comparison helpers ------------------------------------------------------------------------------
def _e32(x32, x64):
    return float((x32.to(F64) - x64).abs().max()) if x64.numel() else 0.0


def _fail(fails, name, msg):
    if fails is None:
        raise AssertionError(f"{name}: {msg}")
    fails.append((name, msg))


def check_elem(name, xk, x64, e32, free=None, ledger=None, fails=None):
    """|X_k - X_64| <= free + MARGIN * e32 per element; ``free``: what needs no fp32 slack (the bf16 half ulp,
    Lip x gap, the erf core's term).  The ledger gets the largest excess over ``free`` in units of e32."""
    assert tuple(xk.shape) == tuple(x64.shape), (name, xk.shape, x64.shape)
    xk = xk.to(F64)
    if not bool(torch.isfinite(xk).all()):
        return _fail(fails, name, "non-finite values stored")
    over = (xk - x64.to(F64)).abs() - (0.0 if free is None else free)
    worst = max(float(over.max()), 0.0) if over.numel() else 0.0
    slack = MARGIN * e32
    if ledger is not None:
        ledger.add(name, worst, e32, slack)
    bad = int((over > slack).sum())
    if bad:
        _fail(fails, name, f"{bad} of {over.numel()} elements over the bound, worst excess {worst:.3e} > 16 * {e32:.3e}")


def check_bits(name, got, want, fails=None):
    if not torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)):
        _fail(fails, name, f"{int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ bitwise")


def interval(v64, slack):
    """The bf16 values a hidden RNE store of a value within ``slack`` of v64 can give: (lo, hi, gap) in fp64.
    (Rounding through fp32 is monotone, so an fp32 value >= v64 - slack never rounds below lo.)"""
    lo, hi = rne_bf16(v64 - slack).to(F64), rne_bf16(v64 + slack).to(F64)
    return lo, hi, hi - lo


def check_share(name, gap, ledger=None, fails=None):
    share = float((gap > 0).double().mean())
    if ledger is not None:
        ledger.note("ambiguous " + name, share)
    if not share < AMBIGUOUS_MAX:
        _fail(fails, name, f"ambiguous share {share:.3f} >= {AMBIGUOUS_MAX}")
    return share


def check_member(name, xk, lo, hi, fails=None):
    xk = xk.to(F64)
    bad = int(((xk < lo) | (xk > hi) | ~torch.isfinite(xk)).sum())
    if bad:
        _fail(fails, name, f"{bad} of {xk.numel()} elements outside the admissible interval")


# ---- forward ------------------------------------------------------------------------------------------------
def forward_ref(c, mode, ledger=None, fails=None, tag="fwd"):
    """Everything of :func:`check_forward` that does not depend on the kernel's outputs (shared by the launchers
    of one case): the admissible pre-activations, the fp64 outputs at their low ends, e32 and the free terms."""
    lg, lgd = lipschitz(mode)
    core = core_term(mode)
    p64, p32 = st_pre(c, F64), st_pre(c, F32)
    lo, gap = [], []
    for i, n in enumerate(("pre_n", "pre_w")):
        e = _e32(p32[i], p64[i])
        l, _, g = interval(p64[i], MARGIN * e)
        if ledger is not None:
            ledger.note(f"e32 {tag}.{n}", e)
        check_share(f"{tag}.{n}", g, ledger, fails)
        lo.append(l)
        gap.append(g)
    o64 = st_out(c, lo[0], lo[1], mode, F64)
    o32 = st_out(c, lo[0].to(F32), lo[1].to(F32), mode, F32)
    ref = {}
    for i, n in enumerate(("gdn", "gdw")):
        drift = lgd * gap[i]
        ref[n] = (o64[i], _e32(o32[i], o64[i]), bf16_half_ulp(o64[i].abs() + drift) + drift + core)
    drift = lg * (gap[0] + gap[1])
    ref["s1"] = (o64[2], _e32(o32[2], o64[2]),
                 bf16_half_ulp(o64[2].abs() + drift) + drift + core * (lo[0].abs() + lo[1].abs()))
    return ref


def check_forward(c, k, mode, layout, ledger=None, fails=None, tag="fwd", ref=None):
    """k: the kernel's gdn / gdw (None: the inference form), s1 (bf16 [B, L, C]) and stats [B, P, 2]."""
    L = c["L"]
    ref = forward_ref(c, mode, ledger, fails, tag) if ref is None else ref
    for n in ("gdn", "gdw", "s1"):
        if k.get(n) is not None:
            check_elem(f"{tag}.{n}(bf16)", k[n], *ref[n], ledger, fails)
    # the LayerNorm partials, from the stored s1
    m64, M64, sq64 = st_stats(k["s1"], L, layout, F64)
    m32, M32, _ = st_stats(k["s1"].to(F32), L, layout, F32)
    if tuple(k["stats"].shape) != (*m64.shape, 2):
        return _fail(fails, f"{tag}.stats", f"shape {tuple(k['stats'].shape)}, expected {(*m64.shape, 2)}")
    check_elem(f"{tag}.mean", k["stats"][..., 0], m64, _e32(m32, m64), None, ledger, fails)
    # M2 = sumsq - sum * mean in fp32 (one pass): its error is that of the two sums, ~2^-24 sumsq, whatever the
    # mean; a two-pass fp32 evaluation is far better once |mean| >> std, so it is the yardstick only where larger
    e2p, ulp = _e32(M32, M64), float((2.0 ** -24 * sq64).max())
    errM = float((k["stats"][..., 1].to(F64) - M64).abs().max())
    if ledger is not None:
        ledger.note(f"{tag}.M2 err / (2^-24 sumsq)", errM / ulp)
        ledger.note(f"{tag}.M2 err / two-pass e32", errM / e2p if e2p > 0 else 0.0)
    check_elem(f"{tag}.M2", k["stats"][..., 1], M64, max(e2p, ulp), None, ledger, fails)


def play_forward(c, mode, layout, dt=F32, rounding=True, mutant=None):
    """The forward chained on its own outputs; returns what a kernel would have stored (plus ``pre``)."""
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    pn, pw = st_pre(c, dt, rounding, mutant, rev=rounding)
    if rounding and mutant != "pre_not_rounded":
        pn, pw = rne_bf16(pn).to(dt), rne_bf16(pw).to(dt)
    dn, dw, s1 = st_out(c, pn, pw, mode, dt, mutant)
    k = dict(gdn=store(dn), gdw=store(dw), s1=store(s1), pre=(pn, pw))
    m, M2, _ = st_stats(k["s1"].to(dt), c["L"], layout, dt, onepass=rounding)
    k["stats"] = torch.stack([m, M2], dim=-1)
    return k


# ---- backward -------------------------------------------------------------------------------------------------
def check_ln1(c, k, got, BM1, eps=EPS, ledger=None, fails=None, tag="ln1"):
    """pbx_ln1_finalize.  k: s1, st1, sums1 (what the launcher was given); got: ds1 (bf16), dgb (after the launch;
    c["dgb0"] before)."""
    L = c["L"]
    a = (c["dh1"], k["s1"], c["g1"])
    d64 = st_ds1(*a, st_ln1_consts(k["st1"], BM1, k["sums1"], L, eps, F64), F64)
    d32 = st_ds1(*a, st_ln1_consts(k["st1"], BM1, k["sums1"], L, eps, F32), F32)
    e = _e32(d32, d64)
    lo, hi, gap = interval(d64, MARGIN * e)
    if ledger is not None:
        ledger.note(f"e32 {tag}.ds1", e)
    check_share(f"{tag}.ds1", gap, ledger, fails)
    check_member(f"{tag}.ds1", got["ds1"], lo, hi, fails)
    check_dgb(c, got["ds1"].to(F64), None, got["dgb"], ledger, fails, tag)


def check_dgb(c, ds1_64, gap, dgb, ledger=None, fails=None, tag="ln1"):
    """dgb - dgb0 = the column sums of dS1 (``gap``: dS1 is hidden, lo was passed: + sum_pos gap)."""
    s64 = c["dgb0"].to(F64) + ds1_64.sum(dim=1)
    s32 = c["dgb0"] + ds1_64.to(F32).sum(dim=1)
    check_elem(f"{tag}.dgb", dgb, s64, _e32(s32, s64), None if gap is None else gap.sum(dim=1), ledger, fails)
    if gap is not None and ledger is not None:
        ledger.note(f"{tag}.dgb largest sum of gaps", float(gap.sum(dim=1).max()))


def dpre_ext(ds1_ext, gd_ext, stored, lo):
    """dpre over the extended rows: the exact products of the halo rows, the kernel's stored rows in the middle."""
    d = rne_bf16(ds1_ext.to(F32) * gd_ext.to(F32))
    if stored is not None:
        d = d.clone()
        d[:, lo:lo + stored.shape[1]] = stored
    return d


def st_dx(c, ds1_mid, dpn_e, dpw_e, dt=F64, rounding=True, mutant=None, rev=False):
    a = (c["L"], c["lo"], c["hi"], dt, 1 if mutant == "dgrad_shift_sign" else -1, rounding, None, rev)
    return ds1_mid.to(dt) + conv_sum(dpn_e, c["wn"], 1, *a) + conv_sum(dpw_e, c["ww"], DIL, *a)


def check_dgrad(c, gdn, gdw, got, ledger=None, fails=None, tag="dgrad4x"):
    """pbx_conv_dgrad4x from c["ds1"] and the GELU' images gdn / gdw (all [B, lo + L + hi, C]); got: dx, dpn, dpw."""
    lo, L = c["lo"], c["L"]
    mid = slice(lo, lo + L)
    for n, gd in (("dpn", gdn), ("dpw", gdw)):
        check_bits(f"{tag}.{n}", got[n], rne_bf16(c["ds1"][:, mid].to(F32) * gd[:, mid].to(F32)), fails)
    dpn_e, dpw_e = dpre_ext(c["ds1"], gdn, got["dpn"], lo), dpre_ext(c["ds1"], gdw, got["dpw"], lo)
    x64 = st_dx(c, c["ds1"][:, mid], dpn_e, dpw_e, F64)
    x32 = st_dx(c, c["ds1"][:, mid], dpn_e, dpw_e, F32)
    check_elem(f"{tag}.dx(bf16)", got["dx"], x64, _e32(x32, x64), bf16_half_ulp(x64), ledger, fails)


def check_dgrad_fin(c, k, BM1, got, eps=EPS, ledger=None, fails=None, tag="dgrad4f"):
    """pbx_conv_dgrad4f (whole sequences).  k: s1, st1, sums1, gdn, gdw as the launcher was given them; got: dx,
    dpn, dpw, dgb.  dS1 is never stored: every output is evaluated at the low end of its admissible interval."""
    L = c["L"]
    a = (c["dh1"], k["s1"], c["g1"])
    d64 = st_ds1(*a, st_ln1_consts(k["st1"], BM1, k["sums1"], L, eps, F64), F64)
    d32 = st_ds1(*a, st_ln1_consts(k["st1"], BM1, k["sums1"], L, eps, F32), F32)
    e = _e32(d32, d64)
    lo, hi, gap = interval(d64, MARGIN * e)
    if ledger is not None:
        ledger.note(f"e32 {tag}.ds1", e)
    check_share(f"{tag}.ds1", gap, ledger, fails)
    for n, gd in (("dpn", k["gdn"]), ("dpw", k["gdw"])):
        g = gd.to(F64)
        v64, drift = lo * g, g.abs() * gap                    # bf16 x bf16: exact in fp32, e32 = 0
        check_elem(f"{tag}.{n}(bf16)", got[n], v64, _e32(lo.to(F32) * gd.to(F32), v64),
                   bf16_half_ulp(v64.abs() + drift) + drift, ledger, fails)
    x64 = st_dx(c, lo, got["dpn"], got["dpw"], F64)
    x32 = st_dx(c, lo.to(F32), got["dpn"], got["dpw"], F32)
    check_elem(f"{tag}.dx(bf16)", got["dx"], x64, _e32(x32, x64), bf16_half_ulp(x64.abs() + gap) + gap, ledger, fails)
    check_dgb(c, lo, gap, got["dgb"], ledger, fails, tag)


def check_embed_dpre(c, ds1, gdn, gdw, got, ledger=None, fails=None, tag="embed_dpre"):
    """pbx_embed_dpre: dpn / dpw bitwise, dE - dE0 = index_add of dS1 over the tokens."""
    for n, gd in (("dpn", gdn), ("dpw", gdw)):
        check_bits(f"{tag}.{n}", got[n], rne_bf16(ds1.to(F32) * gd.to(F32)), fails)
    idx = c["tok"].reshape(-1)
    e64 = c["dE0"].to(F64).index_add(0, idx, ds1.to(F64).reshape(-1, C))
    e32 = c["dE0"].index_add(0, idx, ds1.to(F32).reshape(-1, C))
    check_elem(f"{tag}.dE", got["dE"], e64, _e32(e32, e64), None, ledger, fails)


def play_backward(c, k, BM1, fused, gdn=None, gdw=None, ds1=None, dt=F32, rounding=True, mutant=None, eps=EPS):
    """The backward chained on its own outputs.  ``ds1`` None: dS1 from the LayerNorm-1 finalize of k (s1, st1,
    sums1) -- stored (``fused`` False: ln1_finalize + conv_dgrad4x) or hidden (``fused``: conv_dgrad4f) -- else the
    given [B, lo + L + hi, C] rows (conv_dgrad4x alone).  gdn / gdw default to k's."""
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    L, lo = c["L"], c["lo"]
    got = {}
    gdn = k["gdn"] if gdn is None else gdn
    gdw = k["gdw"] if gdw is None else gdw
    if ds1 is None:
        consts = st_ln1_consts(k["st1"], BM1, k["sums1"], L, eps, dt, mutant)
        ds1 = store(st_ds1(c["dh1"], k["s1"], c["g1"], consts, dt))
        got["dgb"] = c["dgb0"].to(dt) + ds1.to(dt).sum(dim=1)
        if not fused:
            got["ds1"] = ds1
    mid = slice(lo, lo + L)
    dpn_e, dpw_e = store(ds1.to(dt) * gdn.to(dt)), store(ds1.to(dt) * gdw.to(dt))
    got["dpn"], got["dpw"] = dpn_e[:, mid], dpw_e[:, mid]
    got["dx"] = store(st_dx(c, ds1[:, mid], dpn_e, dpw_e, dt, rounding, mutant, rev=rounding))
    return got
