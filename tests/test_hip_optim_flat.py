"""GPU: the flat-arena optimizer kernels (ops/csrc/optim.hip) against plain high-precision references, at
sizes where their grid-stride loops run more than once and at every ``n % 4``.

Grid caps: ``pbx_adam_flat`` and ``pbx_clip_scale_flat`` 2048 blocks (Adam: 2^21 floats per pass),
``pbx_sumsq_flat`` and ``pbx_nonfinite_flag`` 1024 blocks (2^20 floats), ``pbx_fill_flat`` 4096 blocks (2^22).

Adam tolerances.  The oracle is float64 Adam on the kernel's own fp32 inputs of each step
(``step_oracles.adam_ref64``).  The bound is not fitted to the kernel: it is 4 times the worst error that a
float32 numpy emulation of ``adam_one`` (``step_oracles.adam_emul32``) reaches against the same oracle on
the same gradients (2 * 2^21 + 192 elements, p ~ 1e-3 N(0, 1), g ~ 8 N(0, 1), lr = 1e-2,
weight_decay = 0.1, grad_scale = 0.125).  Device ``powf`` and FMA contraction differ from numpy by a few
ulp, and the cancellation in ``1 - beta^t`` amplifies both alike.  e_p is
``max(|p_k - p_64| - 2^-24 |p_64|, 0) / lr``; e_m and e_v are the moment errors relative to the sum of their
absolute terms, in units of 2^-24 (``step_oracles.adam_errors``).

    t        emulation (e_p, e_m, e_v)   bound = 4 x emulation      kernel on an MI355X, worst of the 3 sizes
    1        2.4e-07  1.8  3.9           9.6e-07  7.2  15.6         2.3e-07  1.71 3.84
    2        3.7e-06  2.7  4.5           1.5e-05  10.8 18.0         3.6e-06  1.88 3.64
    3        3.3e-06  2.6  4.3           1.3e-05  10.4 17.2         3.4e-06  1.90 3.67
    11       2.6e-07  2.6  4.2           1.0e-06  10.4 16.8         2.3e-07  1.92 3.58
    12       1.0e-06  2.6  3.9           4.0e-06  10.4 15.6         9.4e-07  1.92 3.32
    13       4.9e-07  2.6  3.8           2.0e-06  10.4 15.2         4.5e-07  1.91 3.26
    1001     1.1e-06  2.6  3.7           4.4e-06  10.4 14.8         9.0e-07  1.92 3.29
    1002     1.1e-06  2.6  3.7           4.4e-06  10.4 14.8         8.6e-07  1.88 2.85
    1003     1.1e-06  2.6  3.3           4.4e-06  10.4 13.2         8.7e-07  1.89 2.66
    100001   9.3e-07  2.6  3.5           3.7e-06  10.4 14.0         7.5e-07  1.92 2.99
    100002   1.2e-06  2.7  3.0           4.8e-06  10.8 12.0         8.4e-07  1.90 2.54
    100003   1.1e-06  2.6  3.1           4.4e-06  10.4 12.4         9.0e-07  1.87 2.60

An off-by-one in the device bias correction costs 0.26 (t = 1) down to 4e-3 (t = 10) in e_p
(tests/test_step_oracles.py::test_adam_tolerance_separates_off_by_one).
"""
import numpy as np
import pytest
import torch

import step_oracles as so
from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam

pytestmark = pytest.mark.gpu

N1 = 1 << 21                                     # one pass of the Adam grid
ADAM_SIZES = (N1, N1 + 64, 2 * N1 + 192)         # one pass exactly, a short second pass, three passes
R1 = 1 << 20                                     # one pass of the 1024-block reductions
RED_SIZES = (R1, R1 + 64, 3 * R1 + 7)
SMALL = (1, 2, 3, 5, 7, 64, 259)                 # n % 4 in {1, 2, 3}: the scalar tail
GUARD = 64
F_SENT = 0x7FC0DEAD                              # a NaN bit pattern: an over-read of it is seen, too
H_SENT = 0x7EEF
EPS24 = 2.0 ** -24
FLT_MAX = 3.4028234663852886e38


def cuda():
    return torch.device("cuda")


def stream():
    return _lib.stream_ptr(cuda())


def guarded(values, dtype=torch.float32):
    """values followed by a guard band of the sentinel pattern, on the GPU."""
    values = torch.as_tensor(values, dtype=dtype).reshape(-1)
    n = values.numel()
    buf = torch.empty(n + GUARD, dtype=dtype, device=cuda())
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(F_SENT)
    else:
        buf.view(torch.int16).fill_(H_SENT)
    buf[:n].copy_(values)
    return buf


def guard_intact(buf, n):
    if buf.dtype == torch.float32:
        return bool(torch.all(buf[n:].view(torch.int32) == F_SENT))
    return bool(torch.all(buf[n:].view(torch.int16) == H_SENT))


def bits_equal(a, b):
    """Bitwise equality (NaN payloads and the sign of zero included)."""
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def bf16_rne_bits(x):
    """Integer round-to-nearest-even of finite fp32 values to bf16 bit patterns (numpy uint16)."""
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def adam_flat(p, g, m, v, shadow, n, hp, skip=None, step_dev=None):
    _lib.call("pbx_adam_flat", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _lib.ptr(shadow), n,
              hp.data_ptr(), _lib.ptr(skip), _lib.ptr(step_dev), stream())


# ---- a / b: Adam against float64, p, m, v and the bf16 shadow after every step ---------------------------
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_matches_float64(n):
    """p, m, v within 4x the float32 emulation's error of float64 Adam (module docstring) and the bf16
    shadow bitwise the round-to-nearest-even of the kernel's own p, after every step: the device step
    counter at t = 1, 2, 3, then three steps each after step_count = 10, 1000, 100000."""
    p = torch.nn.Parameter(torch.from_numpy(so.adam_p0(n)).to(cuda()))
    fa = FusedAdam([p], lr=so.ADAM_LR, betas=so.ADAM_BETAS, eps=so.ADAM_EPS, weight_decay=so.ADAM_WD)
    fa.grad_scale = so.ADAM_GS
    assert fa.arena.numel == n and fa.shadow is not None
    hp = so.adam_hp()
    state = [fa.arena.data.cpu().numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32)]
    failures = []

    def one_step(t):
        g = so.adam_grad(n, t)
        p.grad.copy_(torch.from_numpy(g))
        fa.step()
        torch.cuda.synchronize()
        assert fa.step_count == t and float(fa._step_dev.item()) == float(t)
        hp_dev = fa._hp_dev.cpu().numpy()
        assert np.array_equal(hp_dev[[0, 1, 2, 3, 4, 7]], hp[[0, 1, 2, 3, 4, 7]])
        pk_t = fa.arena.data.cpu()
        pk, mk, vk = pk_t.numpy(), fa.exp_avg.cpu().numpy(), fa.exp_avg_sq.cpu().numpy()
        assert bits_equal(fa.shadow.cpu(), pk_t.to(torch.bfloat16)), f"shadow != bf16(p) at t={t}"
        assert mk.any() and vk.any()
        e = so.adam_errors(pk, mk, vk, state[0], g, state[1], state[2], hp, t)
        bound = tuple(so.ADAM_KERNEL_FACTOR * x for x in so.ADAM_EMUL_TABLE[t])
        print(f"adam n={n} t={t}: kernel e_p={e[0]:.3g} e_m={e[1]:.3g} e_v={e[2]:.3g}  "
              f"bound {bound[0]:.3g} {bound[1]:.3g} {bound[2]:.3g}")
        if not all(x <= b for x, b in zip(e, bound)):
            failures.append((t, e, bound))
        state[:] = [pk, mk, vk]

    for t in (1, 2, 3):
        one_step(t)
    for T in so.ADAM_JUMPS:
        fa.step_count = T
        fa.sync_step_counter()
        for k in (1, 2, 3):
            one_step(T + k)
    assert not failures, failures


def _adversarial_p():
    bits = []
    for h in (0x3F80, 0x3F81, 0x0080, 0x0081, 0x7F00, 0x7F01, 0x4049, 0x1234, 0x1235):
        for sign in (0, 0x8000):
            hi = (h | sign) << 16
            bits += [hi | 0x8000, hi | 0x7FFF, hi | 0x8001]         # the tie (even / odd lower neighbour), +-1 ulp
    bits += [0x00000000, 0x80000000]                                  # +-0
    for s in (0, 0x80000000):                                         # fp32 subnormals
        bits += [s | 0x00000001, s | 0x00007FFF, s | 0x00008000, s | 0x00008001, s | 0x00018000,
                 s | 0x00017FFF, s | 0x00018001, s | 0x007FFFFF, s | 0x007F8000, s | 0x007F7FFF]
        bits += [s | 0x7F7F7FFF, s | 0x7F7F0000]                      # the largest that round to bf16 max
        bits += [s | 0x7F7F8000, s | 0x7F7FFFFF]                      # the smallest / largest that round to inf
    return np.array(bits, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("device_t", [False, True])
def test_adam_passthrough_shadow_rounding(device_t):
    """lr = 0, weight_decay = 0: p comes back bitwise unchanged and shadow is the round-to-nearest-even of
    p, on exact ties (even and odd lower neighbour), one ulp either side of a tie, +-0, fp32 subnormals and
    the values around bf16 max / inf, in the vector body and in the scalar tail.  The gradient is random,
    except that it is positive where p is -0: there -0 - (0 * negative) is +0 in IEEE arithmetic, for any
    Adam."""
    adv = _adversarial_p()
    rng = np.random.default_rng(5)
    p0 = np.concatenate([adv, rng.standard_normal(1031 - 2 * adv.size).astype(np.float32), adv])
    n = p0.size
    assert n == 1031 and n % 4 == 3
    g0 = rng.standard_normal(n).astype(np.float32)
    g0[(p0.view(np.uint32) == 0x80000000)] = 1.0
    want = bf16_rne_bits(p0)
    cpu = torch.from_numpy(p0).to(torch.bfloat16)
    assert np.array_equal(cpu.view(torch.int16).numpy().view(np.uint16), want)     # two references agree
    assert np.isinf(cpu.float().numpy()).sum() == 8 and want[0] == 0x3F80 and want[6] == 0x3F82
    p, g = guarded(p0), torch.from_numpy(g0).to(cuda())
    m, v = guarded(np.zeros(n, np.float32)), guarded(np.zeros(n, np.float32))
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16)
    hp = torch.from_numpy(so.hp_block(0.0, 0.9, 0.999, 1e-8, 0.0, 0.5, 0.5, 0.125)).to(cuda())
    step_dev = torch.full((1,), 3.0, device=cuda()) if device_t else None
    adam_flat(p, g, m, v, shadow, n, hp, None, step_dev)
    torch.cuda.synchronize()
    assert np.array_equal(p[:n].cpu().numpy().view(np.uint32), p0.view(np.uint32)), "p changed under lr = 0"
    got = shadow[:n].cpu().view(torch.int16).numpy().view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(p0.view(np.uint32)[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    assert m[:n].any() and all(guard_intact(b, n) for b in (p, m, v, shadow))


# ---- c: direct launches, the host-supplied bias corrections, tails and guard bands ------------------------
@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("n", SMALL)
def test_adam_direct_host_bias_correction(n, with_shadow):
    """step_dev = nullptr: bias_correction1 / bias_correction2_sqrt are used as the block gives them (odd
    values no t produces), at every n % 4, and nothing after element n is written.

    Bound (reasoned, not measured): the inputs share a sign per element, so nothing cancels and every
    intermediate carries a true relative error: m at most 4 units of 2^-24 (g gs, wd p, their sum,
    (1 - b1) g, b1 m, the sum), v at most 8 (twice g's 1.5, two products, b2 v, the sum), the update
    u = (lr / bc1) m / (sqrt(v) / bc2 + eps) at most 0.5 + 4 + (4 + 1.5) + 1 < 16, and p = p - u one more
    rounding of p.  Recomputed bias corrections would change u by a factor."""
    rng = np.random.default_rng(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    p0 = (sign * 1e-3 * (0.5 + rng.random(n))).astype(np.float32)
    g0 = (sign * 8.0 * (0.1 + rng.random(n))).astype(np.float32)
    m0 = (sign * 0.3 * rng.random(n)).astype(np.float32)
    v0 = (0.7 * rng.random(n)).astype(np.float32)
    hp = so.hp_block(1e-2, 0.9, 0.999, 1e-8, 0.1, bc1=0.37, bc2_sqrt=1.7, grad_scale=0.125)
    p, m, v = guarded(p0), guarded(m0), guarded(v0)
    g = torch.from_numpy(g0).to(cuda())
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16) if with_shadow else None
    adam_flat(p, g, m, v, shadow, n, torch.from_numpy(hp).to(cuda()), None, None)
    torch.cuda.synchronize()
    pk_t = p[:n].cpu()
    pk, mk, vk = pk_t.numpy(), m[:n].cpu().numpy(), v[:n].cpu().numpy()
    p64, _, _ = so.adam_ref64(p0, g0, m0, v0, hp)
    u_max = float(np.max(np.abs(p64 - p0)))
    assert u_max > 1e-4                                    # the update is visible: |u| ~ lr / bc1 * O(0.1)
    e_p, e_m, e_v = so.adam_errors(pk, mk, vk, p0, g0, m0, v0, hp)
    assert e_p <= 16 * EPS24 * u_max / float(hp[0]), (e_p, u_max)
    assert e_m <= 4 and e_v <= 8, (e_m, e_v)
    assert all(guard_intact(b, n) for b in (p, m, v))
    if with_shadow:
        assert bits_equal(shadow[:n].cpu(), pk_t.to(torch.bfloat16)) and guard_intact(shadow, n)


def test_adam_direct_n0_touches_nothing():
    p, m, v = (guarded(np.zeros(0, np.float32)) for _ in range(3))
    shadow = guarded(np.zeros(0, np.float32), torch.bfloat16)
    g = torch.ones(GUARD, device=cuda())
    hp = torch.from_numpy(so.adam_hp()).to(cuda())
    adam_flat(p, g, m, v, shadow, 0, hp, None, None)          # returns 0: _lib.call raises otherwise
    torch.cuda.synchronize()
    assert all(guard_intact(b, 0) for b in (p, m, v, shadow))


# ---- d: range splits on one GPU ---------------------------------------------------------------------------
def test_adam_step_range_splits_are_bitwise():
    """step() against begin_step() + three step_range launches cut at segment boundaries, issued out of
    order, over a multi-tensor arena larger than one pass: p, m, v and the shadow bitwise equal."""
    shapes = [(N1 + 4096,), (300, 1000), (777,), (R1,), (5,)]
    gen = torch.Generator().manual_seed(3)
    init = [1e-3 * torch.randn(s, generator=gen) for s in shapes]

    def make():
        ps = [torch.nn.Parameter(x.clone().to(cuda())) for x in init]
        fa = FusedAdam(ps, lr=1e-2, weight_decay=0.1)
        fa.grad_scale = 0.125
        return ps, fa

    (ps_a, a), (ps_b, b) = make(), make()
    assert a.arena.numel > N1 and a.arena.offsets == b.arena.offsets
    starts = [o for o, _ in a.arena.offsets]
    c1, c2, end = starts[2], starts[4], a.arena.numel
    assert 0 < c1 < c2 < end and end - c2 > N1                 # the last range is itself more than one pass
    for _ in range(2):
        grads = [8.0 * torch.randn(s, generator=gen) for s in shapes]
        for ps in (ps_a, ps_b):
            for q, g in zip(ps, grads):
                q.grad.copy_(g)
        a.step()
        b.begin_step()
        for lo, hi in ((c1, c2), (c2, end), (0, c1)):
            b.step_range(lo, hi)
        torch.cuda.synchronize()
        assert a.step_count == b.step_count and torch.equal(a._step_dev, b._step_dev)
        for x, y in ((a.arena.data, b.arena.data), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq),
                     (a.shadow, b.shadow)):
            assert bits_equal(x, y)
        assert a.exp_avg.abs().sum().item() > 0


# ---- e: the skip flag ----------------------------------------------------------------------------------------
def test_adam_skip_flag_three_passes():
    """skip_flag = 1 leaves p, m, v and the shadow bitwise unchanged over three grid passes; 0 updates
    them.  The step counters are not part of the skip: begin_step() advances the host step_count and the
    device counter on a skipped step as on a taken one, so the two stay equal (and the next taken step's
    bias correction counts the skipped steps)."""
    n = 2 * N1 + 192
    p = torch.nn.Parameter(torch.from_numpy(so.adam_p0(n, seed=1)).to(cuda()))
    fa = FusedAdam([p], lr=1e-2, weight_decay=0.1)
    one = torch.ones(1, dtype=torch.int32, device=cuda())
    zero = torch.zeros(1, dtype=torch.int32, device=cuda())

    def snapshot():
        return [x.clone() for x in (fa.arena.data, fa.exp_avg, fa.exp_avg_sq, fa.shadow)]

    def step(flag, seed):
        p.grad.copy_(torch.from_numpy(so.adam_grad(n, seed, seed=1)))
        fa.skip_flag = flag
        fa.step()
        torch.cuda.synchronize()

    step(zero, 1)                                             # non-zero moments first
    before = snapshot()
    step(one, 2)
    assert all(bits_equal(x, y) for x, y in zip(snapshot(), before))
    step(zero, 3)
    after = snapshot()
    for x, y in zip(after, before):
        assert not torch.equal(x, y)
    # every pass was updated: a moment keeps its old bits only where the new term vanishes in rounding
    # (|g - m| < 6e-7 |m|, |g^2 - v| < 6e-5 v: a handful of 4M elements), never over a whole pass
    for lo, hi in ((0, N1), (N1, 2 * N1), (2 * N1, n)):
        for x, y in zip(after[1:3], before[1:3]):
            assert int((x[lo:hi] == y[lo:hi]).sum()) <= max(8, (hi - lo) // 1000), (lo, hi)
    for flag in (one, one, zero, one):
        step(flag, 4)
    assert fa.step_count == 7 and float(fa._step_dev.item()) == 7.0


# ---- f: sum of squares -----------------------------------------------------------------------------------------
def sumsq(x, n):
    ws = torch.empty(1024, dtype=torch.float32, device=cuda())
    out = torch.full((1,), -1.0, device=cuda())
    _lib.call("pbx_sumsq_flat", x.data_ptr(), n, ws.data_ptr(), out.data_ptr(), stream())
    return out


@pytest.mark.parametrize("n", SMALL + RED_SIZES)
def test_sumsq_matches_float64(n):
    """All summands are non-negative, so the relative error is at most k 2^-24 with k the longest chain of
    roundings: one product, 4 adds per pass over at most 4 passes, the tail, 6 + 3 in the block, 4 + 6 + 3 in
    the final kernel: k < 64.  A large element alone in the second / third pass or in the scalar tail makes
    a skipped pass an error by a factor.  Two calls give the same bits."""
    gen = torch.Generator().manual_seed(n)
    x_cpu = torch.randn(n, generator=gen)
    x = guarded(x_cpu)                                        # the NaN guard band would poison an over-read
    ref = float((x_cpu.double() ** 2).sum())
    a, b = sumsq(x, n), sumsq(x, n)
    assert abs(a.item() - ref) < 64 * EPS24 * ref, (a.item(), ref)
    assert bits_equal(a, b)
    spots = {n - 1, (n // 4) * 4 - 1 if n >= 4 else 0}
    if n > R1:
        spots |= {R1 + 17}
    if n > 3 * R1:
        spots |= {2 * R1 + 33, 3 * R1 + 1}
    for pos in sorted(spots):
        y_cpu = 1e-3 * x_cpu
        y_cpu[pos] = 1e3
        ref = float((y_cpu.double() ** 2).sum())
        got = sumsq(guarded(y_cpu), n).item()
        assert abs(got - ref) < 64 * EPS24 * ref, (pos, got, ref)


# ---- g: clip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 259, (1 << 19) + 64, 2 * N1 + 199])
def test_clip_scale_direct(n):
    """max_norm above the norm: bitwise unchanged (the early return).  Below it every element is within
    4 2^-24 relative of the float64 x max_norm / (sqrt(sumsq) + 1e-6): sqrtf, the sum, the quotient and the
    product round once each.  The grid covers 2^19 elements per pass; 2 * 2^21 + 199 is no multiple of 4."""
    gen = torch.Generator().manual_seed(n)
    x_cpu = torch.randn(n, generator=gen) * 3.0
    ss = torch.tensor([float((x_cpu.double() ** 2).sum())], dtype=torch.float32)
    norm = float(ss.double().sqrt())
    ss_dev = ss.to(cuda())
    x = guarded(x_cpu)
    _lib.call("pbx_clip_scale_flat", x.data_ptr(), n, ss_dev.data_ptr(), float(np.float32(norm * 1.5)), stream())
    torch.cuda.synchronize()
    assert bits_equal(x[:n].cpu(), x_cpu) and guard_intact(x, n)
    max_norm = 0.5
    _lib.call("pbx_clip_scale_flat", x.data_ptr(), n, ss_dev.data_ptr(), max_norm, stream())
    torch.cuda.synchronize()
    ref = x_cpu.double() * (max_norm / (norm + 1e-6))
    err = (x[:n].cpu().double() - ref).abs()
    assert bool(torch.all(err <= 4 * EPS24 * ref.abs())), float((err / ref.abs()).max()) / EPS24
    assert guard_intact(x, n)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_clip_grad_norm_multipass(grad_scale):
    """FusedAdam.clip_grad_norm_ over a three-pass arena against torch's clip_grad_norm_ on the scaled
    gradient (the tolerances of test_clip_grad_norm_gpu_grad_scale)."""
    n = 3 * R1 + 64
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(1)) * 3.0
    p = torch.nn.Parameter(torch.zeros(n, device=cuda()))
    fa = FusedAdam([p], lr=0.1)
    fa.grad_scale = grad_scale
    p.grad.copy_(g0)
    norm = fa.clip_grad_norm_(1.0)
    r = torch.nn.Parameter(torch.zeros(n))
    r.grad = g0 * grad_scale
    norm_t = torch.nn.utils.clip_grad_norm_([r], 1.0)
    torch.testing.assert_close(norm.cpu(), norm_t, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close((p.grad * grad_scale).cpu(), r.grad, rtol=1e-4, atol=1e-6)
    assert float((g0.double() * grad_scale).norm()) > 1.0          # the clip was taken


# ---- h: the non-finite flag, n as the kernel sees it -------------------------------------------------------------
class _Flag:
    def __init__(self):
        self.ws = torch.empty(1024, dtype=torch.int32, device=cuda())
        self.flag = torch.zeros(1, dtype=torch.int32, device=cuda())

    def __call__(self, x, n, bound=float("inf"), accumulate=0, preset=None):
        if preset is not None:
            self.flag.fill_(preset)
        _lib.call("pbx_nonfinite_flag", x.data_ptr(), n, self.ws.data_ptr(), self.flag.data_ptr(), bound,
                  accumulate, stream())
        return int(self.flag.item())


def _flag_positions(n):
    n4 = (n // 4) * 4
    pos = {0, n - 1} | set(range(n4, n))                     # first, last, every scalar-tail element
    if n4:
        pos.add(n4 - 1)                                       # the last vector element
    if n > R1:
        pos.add(R1 + 21)                                      # inside the second pass
    if n > 2 * R1:
        pos.add(2 * R1 + 4099)                                # inside the third pass
    return sorted(pos)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 259, R1 + 64, 3 * R1 + 7])
def test_nonfinite_flag_direct(n):
    """pbx_nonfinite_flag called directly, so n is what the kernel sees (FusedAdam's arena pads every
    segment to 64 elements and never reaches the scalar tail): inf, -inf and nan are found at the first, the
    last, the last vector and every tail element and inside the second and third grid pass; finite 1e30
    noise is not flagged (nor is the NaN guard band after n read); bound = FLT_MAX / 8 flags 5e37 but not
    3e37 at those positions; accumulate = 1 ORs into the flag, accumulate = 0 overwrites it."""
    run = _Flag()
    gen = torch.Generator().manual_seed(n)
    x = guarded(torch.randn(n, generator=gen) * 1e30)
    bound8 = FLT_MAX / 8
    assert run(x, n, preset=1) == 0 and run(x, n, bound8, preset=1) == 0
    for pos in _flag_positions(n):
        keep = x[pos].clone()
        for bad in (float("inf"), float("-inf"), float("nan")):
            x[pos] = bad
            assert run(x, n, preset=0) == 1, (bad, pos)
            assert run(x, n, bound8, preset=0) == 1, (bad, pos)
        for sign in (1.0, -1.0):
            x[pos] = sign * 5e37
            assert run(x, n, preset=1) == 0, pos                   # finite: not flagged without the bound
            assert run(x, n, bound8, preset=0) == 1, pos
            x[pos] = sign * 3e37
            assert run(x, n, bound8, preset=1) == 0, pos
        x[pos] = keep
    assert run(x, n, accumulate=1, preset=1) == 1                  # clean input keeps an earlier 1
    assert run(x, n, accumulate=1, preset=0) == 0
    assert run(x, n, accumulate=0, preset=1) == 0                  # a fresh step overwrites
    x[n - 1] = float("nan")
    assert run(x, n, accumulate=1, preset=0) == 1
    assert run(x, n, accumulate=1) == 1
    assert guard_intact(x, n)


# ---- i: fill and the counters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1.25, -0.0])
@pytest.mark.parametrize("n", [1, 5, 64, (1 << 22) + 71])
def test_fill_flat(n, value):
    """2^22 + 71 is one full pass of the 4096-block grid, a 68-element second pass and a 3-element tail."""
    x = torch.empty(n + GUARD, dtype=torch.float32, device=cuda())
    x.view(torch.int32).fill_(F_SENT)
    _lib.call("pbx_fill_flat", x.data_ptr(), n, value, stream())
    torch.cuda.synchronize()
    assert bits_equal(x[:n], torch.full((n,), value, device=cuda())) and guard_intact(x, n)
    if value == 0.0:
        assert bool(torch.all(x[:n].view(torch.int32) == -(1 << 31)))          # the sign of -0.0 is kept


def test_fill_flat_rejects_unaligned_pointer():
    x = torch.zeros(64, device=cuda())
    with pytest.raises(_lib.HipError):
        _lib.call("pbx_fill_flat", x.data_ptr() + 4, 8, 1.0, stream())
    assert not x.any()
    _lib.call("pbx_fill_flat", x.data_ptr(), 0, 1.0, stream())                 # n = 0: nothing to do
    assert not x.any()


def test_device_counters_are_exact():
    f = torch.zeros(1, device=cuda())
    for _ in range(1000):
        _lib.call("pbx_add_scalar", f.data_ptr(), 1.0, stream())
    assert f.item() == 1000.0
    c = torch.full((1,), 2 ** 32 - 1, dtype=torch.int64, device=cuda())
    _lib.call("pbx_add_i64", c.data_ptr(), 1, stream())
    assert c.item() == 2 ** 32
    _lib.call("pbx_add_i64", c.data_ptr(), 1, stream())
    assert c.item() == 2 ** 32 + 1
    _lib.call("pbx_add_i64", c.data_ptr(), -(2 ** 32 + 2), stream())
    assert c.item() == -1
