"""Stage-wise oracles (torch only, float64 by default) for the two pretraining heads: the local (amino-acid) head
of ``ops/csrc/lhead.hip`` in its five-pass and one-launch forms, and the GO head, the ``EPI_GO`` epilogue of
``ops/csrc/gemm.hip``.

As in tests/global_oracles.py and tests/conv_oracles.py every stage takes ``dt``: ``torch.float64`` gives the oracle
X_64, ``torch.float32`` the yardstick X_32 (the same stage from the same inputs in plain fp32 torch ops), and the
condition on a kernel's tensor X_k is, per element,

    |X_k - X_64| <= free + MARGIN * e32,          e32 = max |X_32 - X_64| over the tensor.

* e32 is floored by ``ulp_floor`` (a tensor of few elements may be hit exactly by fp32 torch) and, for a sum that
  cancels, per element by ``2^-24 sum |terms|`` (:func:`cmp` ``floor``): the softmax runs over the batch, so the
  column sums of dZ are 0 in exact arithmetic and every evaluation of them holds only summation noise.
  dZ = P G - P T is itself such a sum (at B = 1 it cancels entirely: P = 1, T = G): floor 2^-24 (|P G| + |P T|).
* ``free`` is half a bf16 ulp of the fp64 value for a bf16 store; a value computed from a bf16 store the kernel made
  (dh from dz, the GO bias partials from dz) is compared from that store, so nothing has to be carried.  The end to
  end check (:func:`e2e_oracle`) has only the final gradients, so there the admissible width of every bf16 store
  (half ulp + MARGIN e32 of the stored value) is carried through the products as ``sum_k width_k |operand_k|``.
* ``__expf(x)`` is ``v_exp_f32(x * log2(e))``: the product is rounded to fp32 (relative 2^-24) and the constant is
  the fp32 image of log2(e) (relative < 2^-25), so the argument of the base-2 exponential is off by up to
  1.5 * 2^-24 |x log2 e| and the result by the relative 1.5 * 2^-24 |x|, plus one ulp (2^-23) of the instruction
  (:func:`expf_term`).  ``__logf(x)`` is ``v_log_f32(x) * ln 2``: one ulp of |log2 x| and the rounding of the product,
  3 * 2^-24 |log x| in all (:func:`logf_term`).  These terms are derived from the instructions, never from a
  kernel's output; :func:`cmp` applies one only after the plain condition has failed and records that in the ledger.

The GO head's fp64 oracle sends the probability THROUGH fp32 (:func:`st_go`) because the reference does:
``sigmoid -> BCELoss`` in fp32 saturates p to exactly 1.0 (or, where exp overflows, 0.0), the log clamp (-100) and
the zero gradient there are the reference's behaviour and the kernel mirrors them.  Two bands of z are ambiguous in
fp32 (p rounds to 1.0 or not: z in [14, 19]; p denormal or exp overflowing: z in [-92, -80]); :func:`make_go_case`
keeps every logit out of both by construction and asserts it.

:func:`play_local` / :func:`play_go` chain the stages on their own outputs: in fp64 without rounding the plain
expression (validated against autograd in tests/test_head_oracles.py), in fp32 with the bf16 stores a stand-in kernel
(chunks folded in another order than the yardstick sums them), with a ``mutant`` name a deliberately wrong one.
"""
import math

import torch

from conv_oracles import ConvLedger, _e32, _fail, check_elem
from global_oracles import BF16, F32, F64, MARGIN, bf16_half_ulp, rne_bf16, trunc_bf16
from ln_oracles import ulp_floor

CH = 128                 # channels of h
SB = 16                  # samples per chunk / tile (lhead.hip)
PT = 32                  # positions per tile
VP = 32                  # padded vocabulary
GT = 128                 # rows / columns per GO tile (gemm.hip BT)
U24 = 2.0 ** -24
LOG_CLAMP = -100.0
PQ_MIN = 1e-12
BANDS = ((14.0, 19.0), (-92.0, -80.0))      # logits the fp32 sigmoid does not decide

LOCAL_MUTANTS = ("softmax_over_tokens", "weight_as_mask", "mean_over_weighted_rows", "T_dropped", "T_chunk_local",
                 "fold_skips_last_chunk", "pad_rows_counted", "pad_tokens_counted", "logse_twice", "bf16_truncate")
GO_MUTANTS = ("weight_as_mask", "soft_target_as_mask", "no_log_clamp", "grad_unsaturated", "inv_rows_only",
              "pad_cols_not_zeroed", "bias_from_unrounded_dz")


class HeadLedger(ConvLedger):
    """The conv ledger; ``notes`` also keeps the e32 values and the derived intrinsic terms that were needed."""


# ---- derived terms of the hardware transcendentals ----------------------------------------------------------
def expf_term(x, value):
    """|error| of ``__expf(x)`` beyond a correctly rounded exp, as a bound on ``value = exp(x)`` (fp64 tensors)."""
    return value.abs() * (1.5 * U24 * x.abs() + 2.0 ** -23)


def logf_term(value):
    """|error| of ``__logf`` as a bound on ``value = log(x)``."""
    return 3.0 * U24 * value.abs()


def half_ulp(x):
    """global_oracles.bf16_half_ulp, and 0 at an exact 0 (where the masked rows and the saturated columns sit; the
    binade of 0 that frexp reports would grant them 2^-9)."""
    hu = bf16_half_ulp(x)
    return torch.where(x == 0, torch.zeros_like(hu), hu)


# ---- the comparison -----------------------------------------------------------------------------------------
def cmp(name, xk, x64, x32=None, free=None, floor=None, intr=None, e32=None, ledger=None, fails=None, few=False):
    """|X_k - X_64| <= free + MARGIN * max(e32, floor) per element (conv_oracles.check_elem does the asserting).

    ``floor``: the per-element floor of the yardstick of a cancelling sum.  ``few``: e32 also floored by ulp_floor (tensors of few elements only: MS, T, the loss and bias partials).
    ``intr``: a derived intrinsic term (see the module docstring), granted only if the plain condition fails; the
    ledger notes that and its size.  Returns the largest |err| / bound (<= 1: passes), for the tightness tests."""
    x64 = x64.to(F64)
    xk64 = xk.to(F64)
    if not bool(torch.isfinite(x64).all()):
        # a stored input of this stage is so far off that the stage overflows in fp64 (exp of a P >> 1)
        _fail(fails, name, "the oracle of this stage is not finite: the stored tensors it starts from are wrong")
        return float("inf")
    if e32 is None:
        e32 = _e32(x32, x64)
    if few:
        e32 = max(e32, ulp_floor(x64))
    if ledger is not None:
        ledger.note("e32 " + name, e32)
    eff = torch.full_like(x64, e32) if floor is None else torch.clamp(floor.to(F64), min=e32)
    fr = torch.zeros_like(x64) if free is None else (free.to(F64) + torch.zeros_like(x64))
    bound = fr + MARGIN * eff
    err = (xk64 - x64).abs()
    ok = bool(torch.isfinite(xk64).all()) and bool((err <= bound).all())
    if not ok and intr is not None and bool(torch.isfinite(xk64).all()):
        it = intr.to(F64) + torch.zeros_like(x64)
        if bool((err <= bound + it).all()):
            fr, bound = fr + it, bound + it
            if ledger is not None:
                ledger.note("intrinsic term needed " + name, float(it.max()))
    if eff.numel():
        safe = torch.clamp(eff, min=1e-300)
        # in units of the effective yardstick, so that check_elem's scalar e32 is 1
        check_elem(name, (xk64 - x64) / safe, torch.zeros_like(x64), 1.0, fr / safe, ledger, fails)
    if not err.numel():
        return 0.0
    if not bool(torch.isfinite(xk64).all()):
        return float("inf")
    r = err / torch.clamp(bound, min=1e-300)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    return float(r.max())


def exact(name, got, want, fails=None):
    """Bitwise / exact equality of two tensors of one dtype."""
    if tuple(got.shape) != tuple(want.shape) or not torch.equal(got, want):
        n = int((got != want).sum()) if tuple(got.shape) == tuple(want.shape) else -1
        _fail(fails, name, f"{n} elements differ from the exact value")
        return float("inf")
    return 0.0


# ---- inputs -------------------------------------------------------------------------------------------------
def make_local(B, L, V, regime="plain", seed=None):
    """h bf16 [B, L, 128], Wo [V, 128], bo [V], y int64 [B, L], fractional weights [B, L] (about 10 % exact zeros,
    one position with weight 0 for every sample, one sample with weight 0 at every position where B >= 3, and, where
    there is more than one 16 x 32 tile, the whole last tile at weight 0: ``mask_tile`` is its index)."""
    gen = torch.Generator().manual_seed(1000 * L + B + 31 * V if seed is None else seed)
    h = torch.randn(B, L, CH, generator=gen).to(BF16)
    wo = torch.randn(V, CH, generator=gen) * 0.1
    bo = torch.randn(V, generator=gen) * 0.5
    y = torch.randint(0, V, (B, L), generator=gen)
    w = torch.rand(B, L, generator=gen)
    w = torch.where(torch.rand(B, L, generator=gen) < 0.1, torch.zeros_like(w), w)
    if regime == "peaked":
        wo = wo * 8.0
    elif regime == "tied":
        h = h[:1].expand(B, L, CH).contiguous()
    else:
        assert regime == "plain", regime
    c = dict(h=h, wo=wo, bo=bo, y=y, w=w, B=B, L=L, V=V, regime=regime, mask_pos=None, mask_b=None, mask_tile=None)
    if L >= 2:
        c["mask_pos"] = L // 2
        w[:, L // 2] = 0.0
    if B >= 3:
        c["mask_b"] = B // 3
        w[B // 3, :] = 0.0
    if ntiles(B, L) > 1:
        c["mask_tile"] = ntiles(B, L) - 1
        w[(nchunks(B) - 1) * SB:, (L - 1) // PT * PT:] = 0.0
    return c


def make_go_case(B, A, G, ldy=None, lddz=None, wfull=False, seed=None):
    """GO head inputs.  y Bernoulli(0.05) with every 7th column a soft target U(0, 1); per-row weights U(0, 1) with
    30 % zeros (``wfull``: the same expanded to [B, ldy]); saturated bias columns (+25, -25, +95, -95) in the first
    column tile, in the last (partial) column tile and in the last (partial) 8-column group, with |x . w| < 3
    everywhere, so that no logit lies in the bands the fp32 sigmoid does not decide (asserted on the fp64 z)."""
    ldy = A if ldy is None else ldy
    lddz = A if lddz is None else lddz
    gen = torch.Generator().manual_seed(7 * B + A + G if seed is None else seed)
    x = torch.randn(B, G, generator=gen).to(BF16)
    wa = (torch.randn(A, G, generator=gen) * (0.5 / math.sqrt(G))).to(BF16)
    ba = torch.randn(A, generator=gen) * 0.5
    last = (A - 1) // GT * GT
    grp = (A - 1) // 8 * 8
    cols = {}
    for i, v in enumerate((25.0, -25.0, 95.0, -95.0)):
        for c0 in (1 + i, min(last + 1 + i, A - 1), min(grp + i, A - 1), A - 1 - i):
            if 0 <= c0 < A and c0 not in cols:
                cols[c0] = v
    for c0, v in cols.items():
        ba[c0] = v
    y = (torch.rand(B, A, generator=gen) < 0.05).float()
    soft = torch.rand(B, A, generator=gen)
    y[:, ::7] = soft[:, ::7]
    wrow = torch.rand(B, generator=gen)
    wrow = torch.where(torch.rand(B, generator=gen) < 0.3, torch.zeros_like(wrow), wrow)
    z = x.to(F64) @ wa.to(F64).t()
    assert float(z.abs().max()) < 3.0, float(z.abs().max())
    z = z + ba.to(F64)
    for lo, hi in BANDS:
        assert not bool(((z >= lo) & (z <= hi)).any()), (lo, hi)
    ypad = torch.full((B, ldy), 7.0)                     # columns >= A: never read as targets
    ypad[:, :A] = y
    c = dict(x=x, wa=wa, ba=ba, y=y, ypad=ypad, wrow=wrow, B=B, A=A, G=G, ldy=ldy, lddz=lddz,
             sat_cols={v: sorted(k for k, u in cols.items() if u == v) for v in (25.0, -25.0, 95.0, -95.0)})
    c["w"] = wrow[:, None].expand(B, A)
    if wfull:
        wf = torch.full((B, ldy), 3.0)
        wf[:, :A] = c["w"]
        c["wfull"] = wf
    return c


# ---- local head: stages -------------------------------------------------------------------------------------
def wo_img(wo, dt=F64, rounding=True):
    return (rne_bf16(wo) if rounding else wo).to(dt)


def nchunks(B):
    return (B + SB - 1) // SB


def ntiles(B, L):
    return nchunks(B) * ((L + PT - 1) // PT)


def chunk_index(B):
    return torch.arange(B) // SB


def tile_index(B, L):
    """[B, L] tile id of every row: chunk-major, position tile minor (tile_of of lhead.hip)."""
    TP = (L + PT - 1) // PT
    return (torch.arange(B)[:, None] // SB) * TP + torch.arange(L)[None, :] // PT


def st_logits(h, wo, bo, dt=F64, rounding=True):
    """Z [B, L, V] = h . bf16(Wo)^T + bo."""
    return h.to(dt) @ wo_img(wo, dt, rounding).t() + bo.to(dt)


def _by_chunk(x, fn):
    return torch.stack([fn(x[c0:c0 + SB]) for c0 in range(0, x.shape[0], SB)])


def st_chunk_stats(Z, dt=F64):
    """Per 16-sample chunk (max, sum exp(Z - max)) over the chunk's valid samples: two [nch, L, V]."""
    Z = Z.to(dt)
    m = _by_chunk(Z, lambda t: t.max(dim=0).values)
    s = torch.stack([torch.exp(Z[c0:c0 + SB] - m[i]).sum(dim=0) for i, c0 in enumerate(range(0, Z.shape[0], SB))])
    return m, s


def st_stats(Z, dt=F64, raw=False):
    """(M, 1/S) [L, V] over all samples, or the raw (M, S)."""
    Z = Z.to(dt)
    M = Z.max(dim=0).values
    S = torch.exp(Z - M).sum(dim=0)
    return M, (S if raw else 1.0 / S)


def merge_stats(parts, dt=F64):
    """Raw (M, S) images of several shards -> the group's (M, 1/S)."""
    M = torch.stack([p[0].to(dt) for p in parts]).max(dim=0).values
    S = sum(p[1].to(dt) * torch.exp(p[0].to(dt) - M) for p in parts)
    return M, 1.0 / S


def st_ce(Z, M, rS, y, w, Bc, dt=F64, mutant=None, tiles_B=None):
    """From the given Z and (M, 1/S): P, G, per-chunk sum_b G P [nch, L, V], per-tile loss partials [ntiles]
    (already divided by Bc L) and the per-row loss terms.  ``Bc``: the B of the coefficient 1 / (B L)."""
    Z = Z.to(dt)
    B, L, V = Z.shape
    P = torch.exp(Z - M.to(dt)) * rS.to(dt)
    wd = w.to(dt)
    if mutant == "weight_as_mask":
        wd = (wd > 0).to(dt)
    inv = 1.0 / float(wd.sum()) if mutant == "mean_over_weighted_rows" else 1.0 / (Bc * L)
    ex = torch.exp(P)
    se = ex.sum(dim=-1)
    if mutant == "pad_tokens_counted":
        se = se + (VP - V)
    onehot = torch.zeros_like(P).scatter_(-1, y[..., None], 1.0)
    lse = torch.log(se)
    row = wd * ((2.0 * lse if mutant == "logse_twice" else lse) - P.gather(-1, y[..., None])[..., 0])
    G = (wd * inv)[..., None] * (ex / se[..., None] - onehot)
    gp = _by_chunk(G * P, lambda t: t.sum(dim=0))
    gp_abs = _by_chunk((G * P).abs(), lambda t: t.sum(dim=0))
    ti = tile_index(B, L).reshape(-1)
    nt = ntiles(B, L)
    loss_tile = torch.zeros(nt, dtype=dt).index_add_(0, ti, row.reshape(-1)) * inv
    loss_abs = torch.zeros(nt, dtype=dt).index_add_(0, ti, row.abs().reshape(-1)) * inv
    wl = wd * lse                                          # what the error of the hardware log multiplies
    ge = (wd * inv)[..., None] * ex / se[..., None]
    return dict(P=P, G=G, gp=gp, gp_abs=gp_abs, loss_tile=loss_tile, loss_abs=loss_abs, row=row * inv,
                loss_pos=row.sum(dim=0) * inv, loss_pos_abs=row.abs().sum(dim=0) * inv, lse=lse, inv=inv, ge=ge,
                wlse_tile=torch.zeros(nt, dtype=dt).index_add_(0, ti, wl.reshape(-1)) * inv,
                wlse_pos=wl.sum(dim=0) * inv)


def st_T(gp, dt=F64):
    return gp.to(dt).sum(dim=0)


def st_dz(Z, M, rS, T, y, w, Bc, dt=F64, mutant=None):
    """Unrounded dZ [B, L, V] = P (G - T) from the given Z, (M, 1/S) and T ([L, V], or [nch, L, V]: per chunk);
    per-tile column sums [ntiles, V] and the sums of |dZ| they cancel from."""
    ce = st_ce(Z, M, rS, y, w, Bc, dt, mutant)
    B, L, V = ce["P"].shape
    Td = T.to(dt)
    if Td.dim() == 3:
        Td = Td[chunk_index(B)]
    dZ = ce["P"] * (ce["G"] - Td)
    # dZ = P G - P T cancels (entirely at B = 1, where P = 1 and T = G): the floor of its yardstick
    dz_floor = U24 * ((ce["P"] * ce["G"]).abs() + (ce["P"] * Td).abs())
    ti = tile_index(B, L).reshape(-1)
    nt = ntiles(B, L)
    dbo = torch.zeros(nt, V, dtype=dt).index_add_(0, ti, dZ.reshape(-1, V))
    # the terms the column sums of dZ cancel from are P G and P T of every sample
    terms = (ce["P"] * ce["G"]).abs() + (ce["P"] * Td).abs()
    dbo_abs = torch.zeros(nt, V, dtype=dt).index_add_(0, ti, terms.reshape(-1, V))
    # one-launch form: G is evaluated a second time as coef exp(P - log se) with the hardware exp and log
    lse = ce["lse"][..., None]
    dz_intr = ce["P"] * ce["ge"] * (logf_term(lse) + 1.5 * U24 * (ce["P"] - lse).abs() + 2.0 ** -23)
    return dict(dZ=dZ, dbo_tile=dbo, dbo_tile_abs=dbo_abs, dbo_pos=dZ.sum(dim=0), dbo_pos_abs=terms.sum(dim=0),
                dz_floor=dz_floor, dz_intr=dz_intr, G=ce["G"])


def st_dh(dz_bf, wo, dt=F64, rounding=True):
    """dz . bf16(Wo) from a given dz [..., V]."""
    return dz_bf.to(dt) @ wo_img(wo, dt, rounding)


def pad_v(x, fill=0.0):
    """[..., V] -> [..., 32]."""
    out = torch.full((*x.shape[:-1], VP), fill, dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out


# ---- local head: playing the kernel ---------------------------------------------------------------------------
def play_local(c, dt=F32, rounding=True, mutant=None, Bc=None, raw=False):
    """The head chained on its own outputs, in the five-pass layout (Z [B, L, 32], part [nch, L, 32, 2], MS / T
    [L, 32, 2], tpart, loss_part [ntiles], dz [B L, 32], dh [B, L, 128], dbo_part [ntiles, V]) plus the one-launch
    form's ``loss_pos`` [L] and ``dbo_pos`` [L, V].  ``raw``: MS holds (M, S)."""
    B, L, V = c["B"], c["L"], c["V"]
    Bc = B if Bc is None else Bc
    store = (trunc_bf16 if mutant == "bf16_truncate" else rne_bf16) if rounding else (lambda t: t)
    Z = st_logits(c["h"], c["wo"], c["bo"], dt, rounding)
    nch = nchunks(B)
    if mutant == "softmax_over_tokens":
        M = Z.max(dim=-1, keepdim=True).values.expand_as(Z)
        rS = (1.0 / torch.exp(Z - M).sum(dim=-1, keepdim=True)).expand_as(Z)
        cm, cs = st_chunk_stats(Z, dt)
        ce = st_ce(Z, M, rS, c["y"], c["w"], Bc, dt)
        # the coupling term of a softmax over the tokens
        Tfull = (ce["G"] * ce["P"]).sum(dim=-1, keepdim=True).expand_as(Z)
        dZ = ce["P"] * (ce["G"] - Tfull)
        Ms, Ss = st_stats(Z, dt, True)
        T = st_T(ce["gp"], dt)
        ti = tile_index(B, L).reshape(-1)
        dz = dict(dZ=dZ, dbo_tile=torch.zeros(ntiles(B, L), V, dtype=dt).index_add_(0, ti, dZ.reshape(-1, V)),
                  dbo_pos=dZ.sum(dim=0))
        MS = torch.stack([Ms, Ss if raw else 1.0 / Ss], dim=-1)
    else:
        cm, cs = st_chunk_stats(Z, dt)
        if mutant == "pad_rows_counted" and B % SB:
            # rows >= B of the partial chunk read row B - 1 through the clamped address and enter the sum
            cs = cs.clone()
            cs[-1] = cs[-1] + (SB - B % SB) * torch.exp(Z[B - 1] - cm[-1])
        use = nch - 1 if mutant == "fold_skips_last_chunk" and nch > 1 else nch
        # the fold: chunks merged in reverse order (another order than the yardstick's plain sum over B)
        M = cm[:use].max(dim=0).values
        S = sum(cs[i] * torch.exp(cm[i] - M) for i in range(use - 1, -1, -1))
        MS = torch.stack([M, S if raw else 1.0 / S], dim=-1)
        ce = st_ce(Z, M, 1.0 / S, c["y"], c["w"], Bc, dt, mutant)
        T = sum(ce["gp"][i] for i in range(use - 1, -1, -1))
        Tuse = torch.zeros_like(T) if mutant == "T_dropped" else ce["gp"] if mutant == "T_chunk_local" else T
        dz = st_dz(Z, M, 1.0 / S, Tuse, c["y"], c["w"], Bc, dt, mutant)
    dzs = store(dz["dZ"])
    dh = store(st_dh(dzs, c["wo"], dt, rounding))
    z2 = lambda t: torch.stack([t, torch.zeros_like(t)], dim=-1)  # noqa: E731
    return dict(Z=pad_v(Z), part=torch.stack([pad_v(cm), pad_v(cs)], dim=-1), MS=pad_v(MS.transpose(-1, -2)).transpose(-1, -2),
                tpart=z2(pad_v(ce["gp"])), T=z2(pad_v(T)), loss_part=ce["loss_tile"], dz=pad_v(dzs).reshape(B * L, VP),
                dh=dh, dbo_part=dz["dbo_tile"], loss_pos=ce["loss_pos"], dbo_pos=dz["dbo_pos"], dZ=dz["dZ"],
                loss=ce["loss_tile"].sum())


# ---- local head: the conditions ---------------------------------------------------------------------------------
def masked_rows_zero(c, dz, dh, fails, tag):
    """Rows of a position that has weight 0 for EVERY sample get no gradient at all: G = 0 and T[l] = 0.  (A sample
    with weight 0 at every position has G = 0 only: the softmax runs over the batch, so it still receives
    dZ = -P T, which the element-wise conditions check.)"""
    B, L, V = c["B"], c["L"], c["V"]
    if c["mask_pos"] is not None:
        lp = c["mask_pos"]
        if not bool((dz.reshape(B, L, VP)[:, lp].float() == 0).all()):
            _fail(fails, f"{tag}.dz", "a row of the all-masked position is not exactly 0")
        if not bool((dh[:, lp].float() == 0).all()):
            _fail(fails, f"{tag}.dh", "a row of the all-masked position is not exactly 0")


def check_five(c, k, raw=False, Bc=None, MS_used=None, T_used=None, ledger=None, fails=None, tag="five"):
    """Every tensor the five-pass form stores, each stage from the tensors stored for the stage before (CPU
    tensors).  ``raw``: k["MS"] is the raw (M, S) image and ``MS_used`` the merged (M, 1/S) [L, 32, 2] the later
    stages were given; ``T_used``: the summed T [L, 32, 2] stage C was given.  Returns name -> largest err / bound."""
    B, L, V = c["B"], c["L"], c["V"]
    Bc = B if Bc is None else Bc
    a = dict(ledger=ledger, fails=fails)
    r = {}
    y, w = c["y"], c["w"]
    # stage A
    Z64, Z32 = st_logits(c["h"], c["wo"], c["bo"], F64), st_logits(c["h"], c["wo"], c["bo"], F32)
    kZ = k["Z"].reshape(B, L, VP)
    r["Z"] = cmp(f"{tag}.Z", kZ[..., :V], Z64, Z32, **a)
    r["Z_pad"] = exact(f"{tag}.Z[:, V:]", kZ[..., V:], torch.zeros(B, L, VP - V), fails)
    Zs = kZ[..., :V]
    cm64, cs64 = st_chunk_stats(Zs, F64)
    _, cs32 = st_chunk_stats(Zs, F32)
    r["part.max"] = exact(f"{tag}.part.max", k["part"][..., :V, 0], _by_chunk(Zs, lambda t: t.max(dim=0).values), fails)
    r["part.sum"] = cmp(f"{tag}.part.sum", k["part"][..., :V, 1], cs64, cs32, **a)
    M64, S64 = st_stats(Zs, F64, raw)
    _, S32 = st_stats(Zs, F32, raw)
    r["MS.M"] = exact(f"{tag}.MS.M", k["MS"][:, :V, 0], Zs.max(dim=0).values, fails)
    r["MS.S"] = cmp(f"{tag}.MS.S", k["MS"][:, :V, 1], S64, S32, few=True, **a)
    # stage B, from the stored Z and the (M, 1/S) it was given
    ms = (k["MS"] if MS_used is None else MS_used)[:, :V]
    Mk, rSk = ms[..., 0], ms[..., 1]
    ce64, ce32 = st_ce(Zs, Mk, rSk, y, w, Bc, F64), st_ce(Zs, Mk, rSk, y, w, Bc, F32)
    r["tpart"] = cmp(f"{tag}.tpart", k["tpart"][..., :V, 0], ce64["gp"], ce32["gp"], floor=U24 * ce64["gp_abs"], **a)
    r["T"] = cmp(f"{tag}.T", k["T"][:, :V, 0], st_T(ce64["gp"]), st_T(ce32["gp"], F32),
                 floor=U24 * ce64["gp_abs"].sum(dim=0), few=True, **a)
    r["loss_part"] = cmp(f"{tag}.loss_part", k["loss_part"], ce64["loss_tile"], ce32["loss_tile"],
                         floor=U24 * ce64["loss_abs"], intr=logf_term(ce64["wlse_tile"]), few=True, **a)
    # stage C, from the stored Z, the given (M, 1/S) and the T it was given
    Tk = (k["T"] if T_used is None else T_used)[:, :V, 0]
    d64, d32 = st_dz(Zs, Mk, rSk, Tk, y, w, Bc, F64), st_dz(Zs, Mk, rSk, Tk, y, w, Bc, F32)
    kdz = k["dz"].reshape(B, L, VP)
    r["dz"] = cmp(f"{tag}.dz(bf16)", kdz[..., :V], d64["dZ"], d32["dZ"], free=half_ulp(d64["dZ"]),
                  floor=d64["dz_floor"], **a)
    r["dz_pad"] = exact(f"{tag}.dz[:, V:]", kdz[..., V:].float(), torch.zeros(B, L, VP - V), fails)
    h64, h32 = st_dh(kdz[..., :V], c["wo"], F64), st_dh(kdz[..., :V], c["wo"], F32)
    r["dh"] = cmp(f"{tag}.dh(bf16)", k["dh"], h64, h32, free=half_ulp(h64), **a)
    r["dbo_part"] = cmp(f"{tag}.dbo_part", k["dbo_part"], d64["dbo_tile"], d32["dbo_tile"],
                        floor=U24 * d64["dbo_tile_abs"], few=True, **a)
    masked_rows_zero(c, k["dz"], k["dh"], fails, tag)
    # the loss partial of a tile whose rows all have weight 0 is 0.0 (the inputs promise such a tile: not vacuous)
    ti = tile_index(B, L)
    dead = [t for t in range(ntiles(B, L)) if not bool((w[ti == t] != 0).any())]
    assert c.get("mask_tile") is None or c["mask_tile"] in dead, "the inputs hold no all-masked tile"
    r["dead_tiles"] = 0.0
    for t in dead:
        if float(k["loss_part"][t]) != 0.0:
            r["dead_tiles"] = float("inf")
            _fail(fails, f"{tag}.loss_part", f"tile {t} is all masked but its loss partial is {float(k['loss_part'][t])}")
    if B == 1:
        # S = 1 and P = 1 exactly, T is the fp32 image of G, and dZ = P (G - T) is 0 in exact arithmetic.  A kernel
        # that forms G - T from the G it rounded for T stores exactly 0; one whose compiler contracts coef * x - T
        # into one fma stores the exact residual G - fl(G) instead, at most half an fp32 ulp of G (2^-24 |G|), then
        # rounded to bf16 (1 + 2^-8).  Nothing larger is admissible.
        r["S_B1"] = exact(f"{tag}.MS.S (B = 1)", k["MS"][:, :V, 1], torch.ones(L, V), fails)
        lim = U24 * d64["G"].abs() * (1.0 + 2.0 ** -8)
        az = kdz[..., :V].to(F64).abs()
        ratio = torch.where(lim > 0, az / torch.clamp(lim, min=1e-300), torch.where(az > 0, float("inf"), 0.0).to(F64))
        r["dz_B1"] = float(ratio.max())
        if ledger is not None:
            ledger.note(f"{tag}.dz (B = 1) / (2^-24 |G|)", r["dz_B1"])
        if r["dz_B1"] > 1.0:
            _fail(fails, f"{tag}.dz (B = 1)", f"|dz| reaches {r['dz_B1']:.3g} x the rounding residual of G")
    return r


def chain(c, dt, Bc=None):
    """The whole head from the bf16 operands, no rounding (the yardstick / oracle of the one-launch form)."""
    B, L, V = c["B"], c["L"], c["V"]
    Bc = B if Bc is None else Bc
    Z = st_logits(c["h"], c["wo"], c["bo"], dt)
    M, rS = st_stats(Z, dt)
    ce = st_ce(Z, M, rS, c["y"], c["w"], Bc, dt)
    d = st_dz(Z, M, rS, st_T(ce["gp"], dt), c["y"], c["w"], Bc, dt)
    return ce, d


def check_fused(c, k, ledger=None, fails=None, tag="fused", ref=None, Bc=None):
    """The one-launch form (only the outputs exist): k has dz [B L, 32], dh, dbo_pos [L, V], loss_pos [L]."""
    B, L, V = c["B"], c["L"], c["V"]
    a = dict(ledger=ledger, fails=fails)
    (ce64, d64), (ce32, d32) = ref if ref is not None else (chain(c, F64, Bc), chain(c, F32, Bc))
    r = {}
    kdz = k["dz"].reshape(B, L, VP)
    r["dz"] = cmp(f"{tag}.dz(bf16)", kdz[..., :V], d64["dZ"], d32["dZ"], free=half_ulp(d64["dZ"]),
                  floor=d64["dz_floor"], intr=d64["dz_intr"], **a)
    r["dz_pad"] = exact(f"{tag}.dz[:, V:]", kdz[..., V:].float(), torch.zeros(B, L, VP - V), fails)
    h64, h32 = st_dh(kdz[..., :V], c["wo"], F64), st_dh(kdz[..., :V], c["wo"], F32)
    r["dh"] = cmp(f"{tag}.dh(bf16)", k["dh"], h64, h32, free=half_ulp(h64), **a)
    r["loss_part"] = cmp(f"{tag}.loss_part", k["loss_pos"], ce64["loss_pos"], ce32["loss_pos"],
                         floor=U24 * ce64["loss_pos_abs"], intr=logf_term(ce64["wlse_pos"]), few=True, **a)
    # 0 in exact arithmetic: the sharp check of T on this route
    r["dbo_part"] = cmp(f"{tag}.dbo_part", k["dbo_pos"], d64["dbo_pos"], d32["dbo_pos"], floor=U24 * d64["dbo_pos_abs"], few=True, **a)
    masked_rows_zero(c, k["dz"], k["dh"], fails, tag)
    if c["mask_pos"] is not None and float(k["loss_pos"][c["mask_pos"]]) != 0.0:
        _fail(fails, f"{tag}.loss_part", "the all-masked position has a loss partial")
    return r


def check_shard(cfull, lo, k, Bs, ledger=None, fails=None, tag="shard"):
    """One shard (samples lo .. lo + Bs of ``cfull``) of a batch axis shared by several ranks: its dz, dh, dbo_part
    and loss partials against the oracle of the FULL batch, evaluated with the shard's own coefficient 1 / (Bs L)."""
    L, V = cfull["L"], cfull["V"]
    a = dict(ledger=ledger, fails=fails)
    ti = tile_index(Bs, L).reshape(-1)
    nt = ntiles(Bs, L)
    ref = {}
    for dt in (F64, F32):
        ce, d = chain(cfull, dt, Bs)
        dZ, row = d["dZ"][lo:lo + Bs], ce["row"][lo:lo + Bs]
        ref[dt] = dict(dZ=dZ, dz_floor=d["dz_floor"][lo:lo + Bs], dbo=torch.zeros(nt, V, dtype=dt).index_add_(0, ti, dZ.reshape(-1, V)),
                       dbo_abs=torch.zeros(nt, V, dtype=dt).index_add_(0, ti, (d["dz_floor"][lo:lo + Bs] / U24).reshape(-1, V)),
                       loss=torch.zeros(nt, dtype=dt).index_add_(0, ti, row.reshape(-1)),
                       loss_abs=torch.zeros(nt, dtype=dt).index_add_(0, ti, row.abs().reshape(-1)))
    r64, r32 = ref[F64], ref[F32]
    r = {}
    kdz = k["dz"].reshape(Bs, L, VP)
    r["dz"] = cmp(f"{tag}.dz(bf16)", kdz[..., :V], r64["dZ"], r32["dZ"], free=half_ulp(r64["dZ"]),
                  floor=r64["dz_floor"], **a)
    h64, h32 = st_dh(kdz[..., :V], cfull["wo"], F64), st_dh(kdz[..., :V], cfull["wo"], F32)
    r["dh"] = cmp(f"{tag}.dh(bf16)", k["dh"], h64, h32, free=half_ulp(h64), **a)
    r["dbo_part"] = cmp(f"{tag}.dbo_part", k["dbo_part"], r64["dbo"], r32["dbo"], floor=U24 * r64["dbo_abs"], few=True, **a)
    r["loss_part"] = cmp(f"{tag}.loss_part", k["loss_part"], r64["loss"], r32["loss"], floor=U24 * r64["loss_abs"], few=True, **a)
    return r


def shard_of(c, lo, Bs):
    """The inputs of samples lo .. lo + Bs as a case of their own."""
    s = dict(c, B=Bs, mask_b=None, mask_tile=None)
    for n in ("h", "y", "w"):
        s[n] = c[n][lo:lo + Bs].contiguous()
    last = ntiles(Bs, c["L"]) - 1
    if last > 0 and not bool((s["w"][tile_index(Bs, c["L"]) == last] != 0).any()):
        s["mask_tile"] = last
    return s


# ---- GO head ------------------------------------------------------------------------------------------------
def go_tiles(B, A):
    return (B + GT - 1) // GT, (A + GT - 1) // GT


def st_go(x_bf, wa_bf, ba, y, w, dt=F64, mutant=None):
    """z = x wa^T + ba; p, q; loss and gradient per element, loss partials per 128 x 128 tile [tr * tc] (row tile
    major).  fp64: p THROUGH fp32 as the reference's fp32 sigmoid -> BCELoss has it (module docstring), the rest
    fp64 arithmetic on those values.  fp32: plain torch fp32."""
    B, A = x_bf.shape[0], wa_bf.shape[0]
    z = x_bf.to(dt) @ wa_bf.to(dt).t() + ba.to(dt)
    if dt == F64:
        e = torch.exp(-z).to(F32)                          # inf above FLT_MAX
        p = (1.0 / (1.0 + e.to(F64))).to(F32)
        q = (1.0 - p.to(F64)).to(F32)
        p, q = p.to(F64), q.to(F64)
    else:
        p = 1.0 / (1.0 + torch.exp(-z))
        q = 1.0 - p
    yd, wd = y.to(dt), w.to(dt)
    inv = 1.0 / B if mutant == "inv_rows_only" else 1.0 / (B * A)
    if mutant == "weight_as_mask":
        wd = (wd > 0).to(dt)
    lp, lq = torch.log(p), torch.log(q)
    if mutant != "no_log_clamp":
        lp, lq = torch.clamp(lp, min=LOG_CLAMP), torch.clamp(lq, min=LOG_CLAMP)
    ny = (yd == 0).to(dt) if mutant == "soft_target_as_mask" else 1.0 - yd
    # 0 * -inf of the unclamped mutant is NaN, as it would be in a kernel
    loss = wd * -(yd * lp + ny * lq) * inv
    pq = p * q
    g = wd * inv * (p - yd)
    if mutant != "grad_unsaturated":
        g = g * pq / torch.clamp(pq, min=PQ_MIN)
    tr, tc = go_tiles(B, A)
    tid = ((torch.arange(B)[:, None] // GT) * tc + torch.arange(A)[None, :] // GT).reshape(-1)
    lt = torch.zeros(tr * tc, dtype=dt).index_add_(0, tid, loss.reshape(-1))
    la = torch.zeros(tr * tc, dtype=dt).index_add_(0, tid, loss.abs().reshape(-1))
    return dict(z=z, p=p, q=q, g=g, loss=loss, loss_tile=lt, loss_tile_abs=la)


def go_colsum(dz, dt=F64):
    """Per 128-row tile column sums of a given (stored, bf16) dz [B, A]: ([tr, A], the sums of |dz|, rows per tile)."""
    B, A = dz.shape
    tr = (B + GT - 1) // GT
    rid = torch.arange(B) // GT
    s = torch.zeros(tr, A, dtype=dt).index_add_(0, rid, dz.to(dt))
    sa = torch.zeros(tr, A, dtype=F64).index_add_(0, rid, dz.to(F64).abs())
    n = torch.clamp(B - torch.arange(tr) * GT, max=GT).to(F64)
    return s, sa, n


def play_go(c, dt=F32, rounding=True, mutant=None):
    """A stand-in GO head: dz [B, lddz] (pad columns zeroed), dbias_part [tr, A], loss_part [tiles]."""
    o = st_go(c["x"], c["wa"], c["ba"], c["y"], c["w"], dt, mutant)
    store = rne_bf16 if rounding else (lambda t: t)
    B, A, lddz = c["B"], c["A"], c["lddz"]
    dz = torch.zeros(B, lddz, dtype=BF16 if rounding else dt)
    if mutant == "pad_cols_not_zeroed":
        dz[:, A:] = 1.0                                # whatever the buffer held
    dz[:, :A] = store(o["g"])
    src = o["g"] if mutant == "bias_from_unrounded_dz" else dz[:, :A]
    return dict(dz=dz, dbias_part=go_colsum(src, dt)[0], loss_part=o["loss_tile"])


def check_go(c, k, ledger=None, fails=None, tag="go", ref=None):
    """pbx_go_head_fused: k has dz [B, lddz] bf16, dbias_part [tr, A], loss_part [tiles] (CPU tensors)."""
    B, A = c["B"], c["A"]
    a = dict(ledger=ledger, fails=fails)
    o64, o32 = ref if ref is not None else (st_go(c["x"], c["wa"], c["ba"], c["y"], c["w"], F64),
                                            st_go(c["x"], c["wa"], c["ba"], c["y"], c["w"], F32))
    r = {}
    dz = k["dz"][:, :A]
    r["dz"] = cmp(f"{tag}.dz(bf16)", dz, o64["g"], o32["g"], free=half_ulp(o64["g"]), **a)
    r["dz_pad"] = exact(f"{tag}.dz[:, A:lddz]", k["dz"][:, A:].float(), torch.zeros(B, c["lddz"] - A), fails)
    # saturated probabilities: the gradient is exactly 0
    sat = (o64["p"] == 1.0) | (o64["p"] == 0.0)
    assert bool(sat.any())
    if not bool((dz.float()[sat] == 0).all()):
        _fail(fails, f"{tag}.dz", "dz != 0 at a saturated probability")
    # an fp32 sum of n <= 128 exactly representable terms: |err| <= (n - 1) 2^-24 sum |dz|  (derived, not measured)
    s64, sa, n = go_colsum(dz)
    r["dbias_part"] = cmp(f"{tag}.dbias_part", k["dbias_part"], s64, e32=0.0,
                          free=(n - 1)[:, None] * U24 * sa, **a)
    if k.get("loss_part") is not None:
        r["loss_part"] = cmp(f"{tag}.loss_part", k["loss_part"], o64["loss_tile"], o32["loss_tile"],
                             floor=U24 * o64["loss_tile_abs"], intr=logf_term(o64["loss_tile_abs"]), few=True, **a)
    return r


# ---- both heads end to end (HeadsLossFn) ----------------------------------------------------------------------
def e2e_oracle(cl, cg, scale, dt=F64):
    """The gradients HeadsLossFn leaves for ``(scale * total).backward()``, and (fp64 only) the widths the bf16
    stores of dz (GO), dzl (local) and dh admit, carried through the products they enter:
    width = half ulp + MARGIN * e32 of the stored value, free(product) = sum_k width_k |operand_k|."""
    B, L, V = cl["B"], cl["L"], cl["V"]
    s = float(scale)
    ce, d = chain(cl, dt)
    dzl = d["dZ"].reshape(B * L, V)
    hr = cl["h"].to(dt).reshape(B * L, CH)
    og = st_go(cg["x"], cg["wa"], cg["ba"], cg["y"], cg["w"], dt)
    g = og["g"]
    o = dict(loss_local=ce["loss_tile"].sum(), loss_go=og["loss_tile"].sum(), dzl=dzl, dz=g,
             dh=s * st_dh(d["dZ"], cl["wo"], dt), dWo=s * dzl.t() @ hr, dbo=s * dzl.sum(dim=0),
             dg=(s * g) @ cg["wa"].to(dt), dWa=(s * g).t() @ cg["x"].to(dt), dba=s * g.sum(dim=0))
    o["total"] = o["loss_local"] + o["loss_go"]
    o["_abs"] = dict(dbo=abs(s) * dzl.abs().sum(dim=0), dba=abs(s) * g.abs().sum(dim=0))
    return o


def e2e_widths(o64, o32, cl, cg, scale):
    """name -> free term (fp64 tensors) of the end-to-end gradients."""
    s = abs(float(scale))
    unit = float(scale) == 1.0
    wl = half_ulp(o64["dzl"]) + MARGIN * _e32(o32["dzl"], o64["dzl"])        # stored dzl
    wg = half_ulp(o64["dz"]) + MARGIN * _e32(o32["dz"], o64["dz"])           # stored dz
    B, L, V = cl["B"], cl["L"], cl["V"]
    hr = cl["h"].to(F64).reshape(B * L, CH).abs()
    wo = wo_img(cl["wo"]).abs()
    f = {}
    f["dWo"] = s * wl.t() @ hr
    dh_w = (wl @ wo).reshape(B, L, CH)
    dh1 = o64["dh"].abs() / max(s, 1e-300) + dh_w                               # the largest |dh| before the scale
    f["dh"] = s * (dh_w + bf16_half_ulp(dh1)) + (0.0 if unit else bf16_half_ulp(s * (dh1 + bf16_half_ulp(dh1))))
    f["dbo"] = torch.zeros_like(o64["dbo"])                                    # the kernel sums the unrounded dZ
    # the scaled copy of dz is one more bf16 store
    wgs = s * wg + (0.0 if unit else bf16_half_ulp(s * (o64["dz"].abs() + wg)))
    f["dWa"] = wgs.t() @ cg["x"].to(F64).abs()
    f["dg"] = wgs @ cg["wa"].to(F64).abs()
    f["dba"] = s * wg.sum(dim=0)
    return f


def play_e2e(cl, cg, scale, dt=F32):
    """A stand-in HeadsLossFn: the bf16 stores of dz, dzl, dh and of the scaled copies, fp32 products."""
    s = float(scale)
    B, L, V = cl["B"], cl["L"], cl["V"]
    _, d = chain(cl, dt)
    dzl = rne_bf16(d["dZ"]).reshape(B * L, V)
    dh = rne_bf16(st_dh(dzl.reshape(B, L, V), cl["wo"], dt))
    g = rne_bf16(st_go(cg["x"], cg["wa"], cg["ba"], cg["y"], cg["w"], dt)["g"])
    gs = g if s == 1.0 else rne_bf16(g.to(dt) * s)
    return dict(dh=dh if s == 1.0 else rne_bf16(dh.to(dt) * s), dWo=s * (dzl.to(dt).t() @ cl["h"].to(dt).reshape(B * L, CH)),
                dbo=s * d["dZ"].reshape(B * L, V).sum(dim=0), dg=gs.to(dt) @ cg["wa"].to(dt),
                dWa=gs.to(dt).t() @ cg["x"].to(dt), dba=s * g.to(dt).sum(dim=0))


def check_e2e(cl, cg, scale, got, ledger=None, fails=None, tag="e2e", ref=None):
    """dWo, dbo, dWa, dba, dh, dg of ``(scale * total).backward()`` per element against the fp64 chain."""
    o64, o32 = ref if ref is not None else (e2e_oracle(cl, cg, scale, F64), e2e_oracle(cl, cg, scale, F32))
    f = e2e_widths(o64, o32, cl, cg, scale)
    r = {}
    for n in ("dWo", "dbo", "dWa", "dba", "dh", "dg"):
        fl = U24 * o64["_abs"][n] if n in o64["_abs"] else None
        r[n] = cmp(f"{tag}.{n}", got[n], o64[n], o32[n], free=f[n], floor=fl, ledger=ledger, fails=fails,
                   few=n in ("dbo", "dba"))
    if "total" in got:
        r["total"] = cmp(f"{tag}.total", got["total"].reshape(()), o64["total"], o32["total"], few=True, ledger=ledger, fails=fails,
                         intr=logf_term(o64["total"]))
    return r


# ---- the cases of tests/test_hip_heads_exact.py (the CPU stand-in runs the same) ------------------------------
FIVE_SHAPES = [(1, 3, 26), (16, 32, 26), (17, 33, 26), (50, 31, 32), (83, 65, 5), (2049, 2, 26)]
FIVE_CASES = [(s, "plain") for s in FIVE_SHAPES] + [(s, r) for s in ((17, 33, 26), (83, 65, 5)) for r in ("peaked", "tied")]
FUSED_SHAPES = [(1, 3, 26), (33, 5, 26), (512, 3, 26), (513, 2, 26), (1024, 3, 26), (1025, 3, 26), (1536, 7, 26),
                (2047, 5, 26), (2048, 4, 26), (33, 5, 32), (33, 5, 5)]
FUSED_CASES = [(s, "plain") for s in FUSED_SHAPES] + [(s, r) for s in ((33, 5, 26), (513, 2, 26), (2047, 5, 26))
                                                       for r in ("peaked", "tied")]
SHARED_CASE = ((34, 33, 26), 17)                      # two "ranks" of 17
# (B, A, G, ldy, lddz, wfull)
GO_CASES = [(300, 239, 512, 239, 240, False), (300, 239, 512, 240, 240, True), (64, 96, 64, 96, 101, False)]
GO_REAL = (129, 8943, 512)
E2E_CASE = (40, 37, 239, 256)                         # (B, L, A, G)
