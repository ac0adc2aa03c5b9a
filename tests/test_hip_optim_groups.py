"""GPU: the grouped flat-arena Adam launch (``pbx_adam_flat_groups``, ops/csrc/optim.hip) and the layers that
reach it.

Non-decoupled groups are held bitwise to ``pbx_adam_flat`` on each group's ranges alone: both kernels inline
the same ``adam_one`` under the same flags.  The decoupled (AdamW) rule has no flat counterpart, so all three
groups of ``GROUPS`` are also held to float64 the way tests/test_hip_optim_flat.py holds the flat kernel: the
oracle is float64 Adam / AdamW on the kernel's own fp32 inputs of each step (``ref64``), and the bound is
``step_oracles.ADAM_KERNEL_FACTOR`` (4) times the worst error a float32 numpy emulation of the update in the
kernel's operation order (``emul32``) reaches against the same oracle, per group, over the ``EM_N`` elements of
``adam_p0`` / ``adam_grad`` in the A, B, A, C layout below (grad_scale = 0.125).  The figures are
``step_oracles.adam_errors``' (e_p in units of lr, e_m and e_v in units of 2^-24 of the sum of their absolute
terms), with no ``wd p`` term where the decay is decoupled.  ``PYTHONPATH=. python tests/test_hip_optim_groups.py``
(from the repository root) re-measures ``EMUL_TABLE`` on the CPU; the kernel's output is never the reference.
"""
import numpy as np
import pytest
import torch

import step_oracles as so
from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.train.optim import FusedAdam, make_optimizer, param_groups_for

pytestmark = pytest.mark.gpu

N1 = 1 << 21                                     # one pass of the Adam grid (2048 blocks x 256 lanes x 4)
GUARD = 64
F_SENT = 0x7FC0DEAD                              # a NaN bit pattern: an over-read of it is seen, too
H_SENT = 0x7EEF
B_SENT = 0xEE                                    # block-table guard: masked to group 14, which no test defines
EPS24 = 2.0 ** -24
GS = so.ADAM_GS

# (lr, beta1, beta2, eps, weight_decay, decoupled): A is the flat test's configuration, B differs in every
# value, C decays its weights AdamW's way
GROUPS = ((so.ADAM_LR, so.ADAM_BETAS[0], so.ADAM_BETAS[1], so.ADAM_EPS, so.ADAM_WD, False),
          (3e-3, 0.8, 0.99, 1e-6, 0.0, False),
          (1e-2, 0.95, 0.98, 1e-8, 0.1, True))
MASK = sum(1 << i for i, g in enumerate(GROUPS) if g[5])
SEGS = (64, 128, 192, 64)                        # segment sizes, repeated; groups A, B, A, C, repeated
SEG_GROUPS = (0, 1, 0, 2)
EM_N = 7 * 64 * 512                              # 512 repeats of the four segments

# Worst error of emul32 against ref64 per group and step index t (the state carried by the emulation
# itself), rounded up to two digits: (e_p, e_m, e_v).  Re-measured by this file's __main__.
EMUL_TABLE = {
    0: {
        1: (2.2e-07, 1.8, 3.7),
        2: (3.6e-06, 2.3, 4.1),
        3: (3.2e-06, 2.3, 3.9),
        11: (2.2e-07, 2.6, 4),
        12: (9.3e-07, 2.4, 3.2),
        13: (4.3e-07, 2.3, 3.5),
        1001: (8.9e-07, 2.3, 2.8),
        1002: (8.3e-07, 2.4, 3.7),
        1003: (7.9e-07, 2.3, 2.7),
        100001: (9.3e-07, 2.2, 2.7),
        100002: (8.7e-07, 2.4, 2.8),
        100003: (9.2e-07, 2.3, 2.8),
    },
    1: {
        1: (2.8e-07, 1, 1.9),
        2: (4.7e-07, 1.9, 2.4),
        3: (6.1e-07, 1.8, 2.3),
        11: (2.3e-07, 1.9, 2.4),
        12: (1.8e-07, 1.9, 2.1),
        13: (3.4e-07, 1.9, 2.1),
        1001: (6.4e-07, 1.9, 2),
        1002: (4.7e-07, 1.9, 2.1),
        1003: (6.1e-07, 2, 2.2),
        100001: (3.6e-07, 1.9, 2),
        100002: (4.1e-07, 1.8, 1.9),
        100003: (4.2e-07, 1.8, 2),
    },
    2: {
        1: (2.1e-07, 0.96, 1.9),
        2: (3.2e-07, 1.9, 2.3),
        3: (3.9e-07, 1.9, 2.4),
        11: (2.1e-07, 1.8, 2),
        12: (2.1e-07, 1.9, 2.1),
        13: (3.0e-07, 1.9, 1.9),
        1001: (2.8e-07, 1.9, 2),
        1002: (2.5e-07, 1.9, 1.9),
        1003: (3.3e-07, 1.9, 2.1),
        100001: (3.8e-07, 2, 2),
        100002: (4.3e-07, 1.9, 2),
        100003: (4.1e-07, 1.9, 2),
    },
}


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
    elif dtype == torch.uint8:
        buf.fill_(B_SENT)
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


def hp_blocks(bc1=1.0, bc2_sqrt=1.0, groups=GROUPS):
    """[G][8] float32, the AdamHParams block of every group."""
    return np.stack([so.hp_block(lr, b1, b2, eps, wd, bc1, bc2_sqrt, GS) for lr, b1, b2, eps, wd, _ in groups])


def layout(n_elems):
    """(block table uint8[ceil(n / 64)], [(offset, numel, group)]) of the A, B, A, C segment pattern."""
    table, segs, o, i = [], [], 0, 0
    while o < n_elems:
        n = min(SEGS[i % 4], n_elems - o)
        segs.append((o, n, SEG_GROUPS[i % 4]))
        table += [SEG_GROUPS[i % 4]] * ((n + 63) // 64)
        o += SEGS[i % 4]
        i += 1
    return np.array(table, dtype=np.uint8), segs


def adam_flat(p, g, m, v, shadow, n, hp, skip=None, step_dev=None):
    _lib.call("pbx_adam_flat", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _lib.ptr(shadow), n,
              hp.data_ptr(), _lib.ptr(skip), _lib.ptr(step_dev), stream())


def adam_groups(p, g, m, v, shadow, n, hp, n_groups, mask, table, skip=None, step_dev=None):
    _lib.call("pbx_adam_flat_groups", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _lib.ptr(shadow), n,
              hp.data_ptr(), n_groups, mask, table.data_ptr(), _lib.ptr(skip), _lib.ptr(step_dev), stream())


# ---- the float64 oracle, the float32 emulation and the error figures, with the decoupled rule --------------
def ref64(p, g, m, v, hp, t=None, decoupled=False):
    """so.adam_ref64; decoupled: torch.optim.AdamW's order, p *= 1 - lr wd first and no wd p in the gradient."""
    if not decoupled:
        return so.adam_ref64(p, g, m, v, hp, t)
    lr, b1, b2, eps, wd, bc1, bc2s, gs = (float(x) for x in np.asarray(hp, dtype=np.float32))
    if t is not None:
        bc1, bc2s = 1.0 - b1 ** float(t), np.sqrt(1.0 - b2 ** float(t))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    p = p * (1.0 - lr * wd)
    g = g * gs
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))
    return p, m, v


def emul32(p, g, m, v, hp, t=None, decoupled=False):
    """so.adam_emul32; decoupled: adam_one_decoupled in numpy float32, operation by operation (no FMA)."""
    if not decoupled:
        return so.adam_emul32(p, g, m, v, hp, t)
    f = np.float32
    lr, b1, b2, eps, wd, bc1, bc2s, gs = (f(x) for x in np.asarray(hp, dtype=np.float32))
    if t is not None:
        bc1 = f(1.0) - np.power(b1, f(t), dtype=np.float32)
        bc2s = np.sqrt(f(1.0) - np.power(b2, f(t), dtype=np.float32), dtype=np.float32)
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    p = p * (f(1.0) - lr * wd)
    g = g * gs
    m = b1 * m + (f(1.0) - b1) * g
    v = b2 * v + (f(1.0) - b2) * g * g
    denom = np.sqrt(v) / bc2s + eps
    p = p - (lr / bc1) * (m / denom)
    assert p.dtype == np.float32 and m.dtype == np.float32 and v.dtype == np.float32
    return p, m, v


def errors(pk, mk, vk, p, g, m, v, hp, t=None, decoupled=False):
    """so.adam_errors' three figures; decoupled: against ref64's AdamW and without the wd p term."""
    if not decoupled:
        return so.adam_errors(pk, mk, vk, p, g, m, v, hp, t)
    hp = np.asarray(hp, dtype=np.float32)
    lr, b1, b2, _, _, _, _, gs = (float(x) for x in hp)
    p64, m64, v64 = ref64(p, g, m, v, hp, t, True)
    e_p = float(np.max(np.maximum(np.abs(pk - p64) - EPS24 * np.abs(p64), 0.0))) / lr
    ga = np.abs(g * np.float64(gs))
    sm = np.abs(b1 * m.astype(np.float64)) + (1.0 - b1) * ga
    sv = np.abs(b2 * v.astype(np.float64)) + (1.0 - b2) * ga * ga
    tiny = np.finfo(np.float64).tiny
    e_m = float(np.max(np.abs(mk - m64) / np.maximum(sm, tiny))) / EPS24
    e_v = float(np.max(np.abs(vk - v64) / np.maximum(sv, tiny))) / EPS24
    return e_p, e_m, e_v


def group_index(n_elems):
    """Element indices of every group in the A, B, A, C layout."""
    _, segs = layout(n_elems)
    return [np.concatenate([np.arange(o, o + n) for o, n, g in segs if g == gi]) for gi in range(len(GROUPS))]


def measure_table(n=EM_N, seed=0, steps=so.ADAM_STEPS):
    """{group: {t: (e_p, e_m, e_v)}} of the emulation."""
    hps, idx = hp_blocks(), group_index(n)
    p, m, v = so.adam_p0(n, seed), np.zeros(n, np.float32), np.zeros(n, np.float32)
    out = {gi: {} for gi in range(len(GROUPS))}
    for t in steps:
        g = so.adam_grad(n, t, seed)
        for gi, ix in enumerate(idx):
            dec = GROUPS[gi][5]
            pk, mk, vk = emul32(p[ix], g[ix], m[ix], v[ix], hps[gi], t, dec)
            out[gi][t] = errors(pk, mk, vk, p[ix], g[ix], m[ix], v[ix], hps[gi], t, dec)
            p[ix], m[ix], v[ix] = pk, mk, vk
    return out


# ---- a: bitwise against the flat kernel -----------------------------------------------------------------------
def _random_state(n, seed):
    rng = np.random.default_rng(seed)
    return ((1e-3 * rng.standard_normal(n)).astype(np.float32), (8.0 * rng.standard_normal(n)).astype(np.float32),
            (0.3 * rng.standard_normal(n)).astype(np.float32), (0.7 * rng.random(n)).astype(np.float32))


def _flat_per_segment(p0, g0, m0, v0, segs, hps, step_dev):
    """pbx_adam_flat on every segment alone, with its group's block: the bitwise reference."""
    n = p0.size
    p, m, v = (torch.from_numpy(x.copy()).to(cuda()) for x in (p0, m0, v0))
    g = torch.from_numpy(g0).to(cuda())
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=cuda())
    for o, k, gi in segs:
        adam_flat(p[o:], g[o:], m[o:], v[o:], shadow[o:], k, hps[gi], None, step_dev)
    torch.cuda.synchronize()
    return p, m, v, shadow


@pytest.mark.parametrize("device_t", [False, True])
def test_groups_bitwise_flat_per_group(device_t):
    """Segments of 64, 128, 192 and 64 elements in groups A, B, A, C, 8 times over (four workgroups): some
    wave's four blocks are in three groups.  All groups non-decoupled: p, m, v and the shadow of every
    segment are bitwise what pbx_adam_flat gives on that segment alone with its group's block, with the
    host's (odd) bias corrections and with the device's."""
    n = 8 * sum(SEGS)
    table_np, segs = layout(n)
    assert any(len(set(table_np[b:b + 4])) == 3 for b in range(0, len(table_np) - 3, 4))
    p0, g0, m0, v0 = _random_state(n, 11)
    hps_np = hp_blocks(bc1=0.37, bc2_sqrt=1.7)
    hps = torch.from_numpy(hps_np).to(cuda())
    step_dev = torch.full((1,), 3.0, device=cuda()) if device_t else None
    want = _flat_per_segment(p0, g0, m0, v0, segs, hps, step_dev)
    p, m, v = guarded(p0), guarded(m0), guarded(v0)
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16)
    adam_groups(p, torch.from_numpy(g0).to(cuda()), m, v, shadow, n, hps, 3, 0, guarded(table_np, torch.uint8),
                None, step_dev)
    torch.cuda.synchronize()
    for name, got, ref in zip("pmvs", (p, m, v, shadow), want):
        assert bits_equal(got[:n], ref), name
        assert guard_intact(got, n), name
    assert not torch.equal(p[:n].cpu(), torch.from_numpy(p0))
    # the three groups really differ: with group A's block everywhere the result is another
    other = _flat_per_segment(p0, g0, m0, v0, [(o, k, 0) for o, k, _ in segs], hps, step_dev)
    assert not torch.equal(other[0], want[0])


# ---- b: edge sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 259, 1031])
def test_groups_edge_sizes(n, with_shadow):
    """A table of ceil(n / 64) entries whose groups cycle A, B, C block by block; the last block is partial and
    n % 4 elements go through the scalar tail.  A and B blocks are bitwise pbx_adam_flat on the block alone.
    C is decoupled and is held to float64 by a reasoned bound, as
    test_hip_optim_flat.py::test_adam_direct_host_bias_correction: inputs share a sign per element, so m
    carries at most 3 + 1 units of 2^-24 (g gs, (1 - b1) g, b1 m, the sum), v at most 8, the update u at
    most 16 of u, and p (1 - lr wd) at most 1.5 of p before the final subtraction's own rounding.  Nothing
    after element n is written."""
    rng = np.random.default_rng(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    p0 = (sign * 1e-3 * (0.5 + rng.random(n))).astype(np.float32)
    g0 = (sign * 8.0 * (0.1 + rng.random(n))).astype(np.float32)
    m0 = (sign * 0.3 * rng.random(n)).astype(np.float32)
    v0 = (0.7 * rng.random(n)).astype(np.float32)
    nb = (n + 63) // 64
    table_np = (np.arange(nb) % 3).astype(np.uint8)
    segs = [(64 * b, min(64, n - 64 * b), int(table_np[b])) for b in range(nb)]
    hps_np = hp_blocks(bc1=0.37, bc2_sqrt=1.7)
    hps = torch.from_numpy(hps_np).to(cuda())
    want = _flat_per_segment(p0, g0, m0, v0, segs, hps, None)
    p, m, v = guarded(p0), guarded(m0), guarded(v0)
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16) if with_shadow else None
    adam_groups(p, torch.from_numpy(g0).to(cuda()), m, v, shadow, n, hps, 3, MASK, guarded(table_np, torch.uint8))
    torch.cuda.synchronize()
    pk_t = p[:n].cpu()
    pk, mk, vk = pk_t.numpy(), m[:n].cpu().numpy(), v[:n].cpu().numpy()
    for o, k, gi in segs:
        sl = slice(o, o + k)
        if not GROUPS[gi][5]:
            for got, ref in zip((p, m, v), want):
                assert bits_equal(got[sl], ref[sl]), (o, gi)
            continue
        hp = hps_np[gi]
        p64, _, _ = ref64(p0[sl], g0[sl], m0[sl], v0[sl], hp, None, True)
        u_max = float(np.max(np.abs(p64 - p0[sl] * (1.0 - float(hp[0]) * float(hp[4])))))
        assert u_max > 1e-4
        e_p, e_m, e_v = errors(pk[sl], mk[sl], vk[sl], p0[sl], g0[sl], m0[sl], v0[sl], hp, None, True)
        assert e_p <= EPS24 * (16 * u_max + 2 * float(np.max(np.abs(p0[sl])))) / float(hp[0]), (o, e_p, u_max)
        assert e_m <= 4 and e_v <= 8, (o, e_m, e_v)
    assert all(guard_intact(b, n) for b in (p, m, v))
    if with_shadow:
        assert bits_equal(shadow[:n].cpu(), pk_t.to(torch.bfloat16)) and guard_intact(shadow, n)


def test_groups_n0_touches_nothing():
    p, m, v = (guarded(np.zeros(0, np.float32)) for _ in range(3))
    shadow = guarded(np.zeros(0, np.float32), torch.bfloat16)
    g = torch.ones(GUARD, device=cuda())
    hps = torch.from_numpy(hp_blocks()).to(cuda())
    adam_groups(p, g, m, v, shadow, 0, hps, 3, MASK, guarded(np.zeros(0, np.uint8), torch.uint8))
    torch.cuda.synchronize()
    assert all(guard_intact(b, 0) for b in (p, m, v, shadow))


@pytest.mark.parametrize("n_groups", [0, 17, -1])
def test_groups_bad_count_is_an_error(n_groups):
    """n_groups outside 1..16: hipErrorInvalidValue, nothing launched, the buffers as they were."""
    n = 259
    p0, g0, m0, v0 = _random_state(n, 2)
    p, m, v = guarded(p0), guarded(m0), guarded(v0)
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16)
    hps = torch.from_numpy(hp_blocks(groups=GROUPS * 6)).to(cuda())             # 18 blocks: no read past them either way
    table = guarded(np.zeros((n + 63) // 64, np.uint8), torch.uint8)
    with pytest.raises(_lib.HipError):
        adam_groups(p, torch.from_numpy(g0).to(cuda()), m, v, shadow, n, hps, n_groups, 0, table)
    torch.cuda.synchronize()
    for got, ref in zip((p, m, v), (p0, m0, v0)):
        assert bits_equal(got[:n].cpu(), torch.from_numpy(ref)) and guard_intact(got, n)
    assert not shadow[:n].view(torch.int16).any() and guard_intact(shadow, n)


# ---- c: a range that starts mid-arena -----------------------------------------------------------------------
def test_groups_range_from_mid_arena():
    """start = 64 k with the table pointer advanced by k: the same elements of a whole-arena launch, bitwise;
    nothing before start is touched.  k = 5 starts inside a 192-element segment, mid-wave."""
    n, k = 8 * sum(SEGS) + 3, 5
    table_np, _ = layout(n)
    p0, g0, m0, v0 = _random_state(n, 4)
    hps = torch.from_numpy(hp_blocks()).to(cuda())
    step_dev = torch.full((1,), 2.0, device=cuda())
    g = torch.from_numpy(g0).to(cuda())
    table = guarded(table_np, torch.uint8)

    def run(start):
        p, m, v = guarded(p0), guarded(m0), guarded(v0)
        shadow = guarded(np.zeros(n, np.float32), torch.bfloat16)
        adam_groups(p[start:], g[start:], m[start:], v[start:], shadow[start:], n - start, hps, 3, MASK,
                    table[start // 64:], None, step_dev)
        torch.cuda.synchronize()
        return p, m, v, shadow

    whole, part = run(0), run(64 * k)
    for a, b, x0 in zip(whole, part, (p0, m0, v0, np.zeros(n, np.float32))):
        assert bits_equal(a[64 * k:n], b[64 * k:n]) and guard_intact(b, n)
        first = torch.from_numpy(x0[:64 * k]).to(b.dtype)
        assert bits_equal(b[:64 * k].cpu(), first)
    assert not torch.equal(whole[0][:64 * k].cpu(), torch.from_numpy(p0[:64 * k]))


# ---- d: more than one grid pass, and step_range splits ----------------------------------------------------------
def test_groups_multipass_step_range_splits_are_bitwise():
    """2 * 2^21 + 192 elements (three grid passes) in two groups split at block 32769 (odd): step() against
    begin_step() and three step_range launches cut inside both groups, out of order: p, m, v and the shadow
    bitwise equal.  The second group has lr = 0 and no decay: its parameters keep their bits (the table is
    right beyond the first pass), its moments move."""
    n_a, n_b = N1 + 64, N1 + 128
    assert (n_a // 64) % 2 == 1 and n_a + n_b == 2 * N1 + 192
    gen = torch.Generator().manual_seed(3)
    init = [1e-3 * torch.randn(n_a, generator=gen), 1e-3 * torch.randn(n_b, generator=gen)]

    def make():
        ps = [torch.nn.Parameter(x.clone().to(cuda())) for x in init]
        # the arena holds the concatenated groups in reverse: ps[0] (n_a elements, group 1) comes first
        fa = FusedAdam([dict(params=[ps[1]], lr=0.0, betas=(0.8, 0.99)),
                        dict(params=[ps[0]], lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True)])
        fa.grad_scale = 0.125
        return ps, fa

    (ps_a, a), (ps_b, b) = make(), make()
    assert a.arena.numel == 2 * N1 + 192 and a.arena.offsets == [(0, n_a), (n_a, n_b)]
    assert a._hp_dev.numel() == 16 and a._decoupled_mask() == 2
    table = a._block_group.cpu()
    assert table.numel() == a.arena.numel // 64 and int(table[:n_a // 64].min()) == 1 \
        and int(table[n_a // 64:].max()) == 0
    c1, c2, end = 64 * 1001, N1 + 64 * 7, a.arena.numel
    assert c1 < n_a < c2
    for _ in range(2):
        grads = [8.0 * torch.randn(x.shape, generator=gen) for x in init]
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
    assert bits_equal(ps_a[1].detach().cpu(), init[1])                   # lr = 0: untouched in every pass
    assert bits_equal(a.shadow[n_a:].cpu(), init[1].to(torch.bfloat16))
    for lo, hi in ((0, n_a), (n_a, 2 * N1), (2 * N1, end)):
        assert int((a.exp_avg[lo:hi] == 0).sum()) <= 8, (lo, hi)
    moved = ps_a[0].detach().cpu() != init[0]
    assert float(moved.float().mean()) > 0.99


# ---- e: three groups against float64, bound from the emulation table ------------------------------------------
def test_groups_match_float64():
    """p, m, v of every group within 4x the float32 emulation's error of float64 Adam / AdamW (module
    docstring), the shadow bitwise the bf16 of the kernel's own p: the device step counter at t = 1, 2, 3,
    then three steps each after 10, 1000, 100000."""
    n = EM_N
    table_np, _ = layout(n)
    idx = group_index(n)
    hps_np = hp_blocks()
    hps = torch.from_numpy(hps_np).to(cuda())
    table = guarded(table_np, torch.uint8)
    p, m, v = guarded(so.adam_p0(n)), guarded(np.zeros(n, np.float32)), guarded(np.zeros(n, np.float32))
    shadow = guarded(np.zeros(n, np.float32), torch.bfloat16)
    step_dev = torch.zeros(1, device=cuda())
    state = [p[:n].cpu().numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32)]
    failures = []
    for t in so.ADAM_STEPS:
        g = so.adam_grad(n, t)
        step_dev.fill_(float(t))
        adam_groups(p, torch.from_numpy(g).to(cuda()), m, v, shadow, n, hps, 3, MASK, table, None, step_dev)
        torch.cuda.synchronize()
        pk_t = p[:n].cpu()
        pk, mk, vk = pk_t.numpy(), m[:n].cpu().numpy(), v[:n].cpu().numpy()
        assert bits_equal(shadow[:n].cpu(), pk_t.to(torch.bfloat16)), f"shadow != bf16(p) at t={t}"
        for gi, ix in enumerate(idx):
            e = errors(pk[ix], mk[ix], vk[ix], state[0][ix], g[ix], state[1][ix], state[2][ix], hps_np[gi], t,
                       GROUPS[gi][5])
            bound = tuple(so.ADAM_KERNEL_FACTOR * x for x in EMUL_TABLE[gi][t])
            print(f"adam groups g={gi} t={t}: kernel e_p={e[0]:.3g} e_m={e[1]:.3g} e_v={e[2]:.3g}  "
                  f"bound {bound[0]:.3g} {bound[1]:.3g} {bound[2]:.3g}")
            if not all(x <= b for x, b in zip(e, bound)):
                failures.append((gi, t, e, bound))
        state[:] = [pk, mk, vk]
    assert all(guard_intact(b, n) for b in (p, m, v, shadow))
    assert not failures, failures


# ---- f: the skip flag -------------------------------------------------------------------------------------------
def _small_model():
    from proteinbert_pytorch_replication_amd.models import ProteinBERT
    torch.manual_seed(0)
    return ProteinBERT(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8, num_heads=4,
                       num_blocks=2, device="cuda", backend="torch")      # only its arena layout is used


def test_groups_skip_flag():
    """A set skip flag leaves p, m, v and the shadow of every group bitwise unchanged, and the step counters
    still advance (host and device stay equal); a cleared one updates all of them."""
    model = _small_model()
    fa = make_optimizer(model, groups=param_groups_for(model, 1e-2, weight_decay=0.1,
                                                       lr_scale={"proteinBERT_blocks.": 0.5}),
                        decoupled_weight_decay=True)
    assert len(fa.param_groups) == 4 and fa._decoupled_mask() == 15
    n = fa.arena.numel
    one = torch.ones(1, dtype=torch.int32, device=cuda())
    zero = torch.zeros(1, dtype=torch.int32, device=cuda())

    def snapshot():
        return [x.clone() for x in (fa.arena.data, fa.exp_avg, fa.exp_avg_sq, fa.shadow)]

    def step(flag, t):
        fa.arena.grad.copy_(torch.from_numpy(so.adam_grad(n, t, seed=1)))
        fa.skip_flag = flag
        fa.step()
        torch.cuda.synchronize()

    step(zero, 1)
    before = snapshot()
    step(one, 2)
    assert all(bits_equal(x, y) for x, y in zip(snapshot(), before))
    assert fa.step_count == 2 and float(fa._step_dev.item()) == 2.0
    step(zero, 3)
    after = snapshot()
    table = fa._block_group.repeat_interleave(64)
    for gi in range(4):
        sel = table == gi
        assert int(sel.sum()) > 0
        for x, y in zip(after, before):
            assert not torch.equal(x[sel], y[sel]), gi
    assert fa.step_count == 3 and float(fa._step_dev.item()) == 3.0


# ---- g: the whole optimizer on a model's arena ------------------------------------------------------------------
def test_fused_adam_two_groups_on_a_model():
    """A two-group FusedAdam over a small ProteinBERT's arena, the biases and LayerNorm affines at lr = 0, for
    3 steps.  The model gives the layout (the groups alternate every few blocks); the parameters and the
    gradients are adam_p0 / adam_grad, for which group A's bound of the emulation table was measured (over
    more elements than this arena has).  The lr = 0 group keeps its parameters bitwise and its moments
    move; the other group is within the bound of float64 Adam."""
    model = _small_model()
    groups = param_groups_for(model, so.ADAM_LR, weight_decay=so.ADAM_WD)
    assert len(groups) == 2 and groups[1]["weight_decay"] == 0.0
    groups[1]["lr"] = 0.0
    fa = make_optimizer(model, groups=groups, betas=so.ADAM_BETAS, eps=so.ADAM_EPS)     # the model's own layout
    fa.grad_scale = GS
    n = fa.arena.numel
    assert n <= EM_N and fa.shadow is not None and fa._decoupled_mask() == 0
    fa.arena.data.copy_(torch.from_numpy(so.adam_p0(n)))
    table = fa._block_group.cpu().numpy().repeat(64)
    ix = [np.nonzero(table == gi)[0] for gi in (0, 1)]
    assert ix[0].size > 0 and ix[1].size > 0 and int(np.abs(np.diff(table.astype(np.int8))).sum()) > 8
    hp = so.adam_hp()
    state = [fa.arena.data.cpu().numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32)]
    p_start = state[0].copy()
    for t in (1, 2, 3):
        g = so.adam_grad(n, t)
        fa.arena.grad.copy_(torch.from_numpy(g))
        fa.step()
        torch.cuda.synchronize()
        assert np.array_equal(fa._hp_dev.cpu().numpy().reshape(2, 8)[0, [0, 1, 2, 3, 4, 7]], hp[[0, 1, 2, 3, 4, 7]])
        pk_t = fa.arena.data.cpu()
        pk, mk, vk = pk_t.numpy(), fa.exp_avg.cpu().numpy(), fa.exp_avg_sq.cpu().numpy()
        assert bits_equal(fa.shadow.cpu(), pk_t.to(torch.bfloat16))
        a = ix[0]
        e = so.adam_errors(pk[a], mk[a], vk[a], state[0][a], g[a], state[1][a], state[2][a], hp, t)
        bound = tuple(so.ADAM_KERNEL_FACTOR * x for x in EMUL_TABLE[0][t])
        print(f"two-group optimizer t={t}: e_p={e[0]:.3g} e_m={e[1]:.3g} e_v={e[2]:.3g}  bound {bound}")
        assert all(x <= b for x, b in zip(e, bound)), (t, e, bound)
        state[:] = [pk, mk, vk]
    z = ix[1]
    assert np.array_equal(state[0][z].view(np.uint32), p_start[z].view(np.uint32))
    assert np.count_nonzero(state[1][z]) > 0.99 * z.size and np.count_nonzero(state[2][z]) > 0.99 * z.size
    assert not np.array_equal(state[0][ix[0]], p_start[ix[0]])


# ---- h: the captured step -----------------------------------------------------------------------------------------
def _graph_setup():
    from proteinbert_pytorch_replication_amd.data import SyntheticUniRefGO
    from proteinbert_pytorch_replication_amd.models import ProteinBERT
    from proteinbert_pytorch_replication_amd.train.step import PretrainStep
    torch.manual_seed(0)
    m = ProteinBERT(sequences_length=128, num_annotations=512, local_dim=128, global_dim=256, key_dim=64,
                    num_heads=4, num_blocks=2, device="cuda", backend="hip")
    groups = param_groups_for(m, 1e-3, weight_decay=0.1)
    groups[1]["lr"] = 5e-4
    opt = make_optimizer(m, groups=groups, decoupled_weight_decay=True)
    assert len(opt.param_groups) == 2
    return m, opt, PretrainStep(m, opt), SyntheticUniRefGO(128, 512, 8, "cuda", seed=11)


def test_graphed_step_two_groups_matches_eager_bitwise():
    """After tests/test_graph_step.py, in deterministic mode (no float atomics in the backward): two eager
    warmup steps and three replays of the captured two-group step equal five eager steps bitwise, with both
    groups' learning rates changed before every one of the last three steps, as a scheduler would
    (prepare() pushes them outside the capture)."""
    from proteinbert_pytorch_replication_amd.train.step import GraphedStep
    from proteinbert_pytorch_replication_amd.utils import determinism
    base, factor = (1e-3, 5e-4), {3: 0.5, 4: 0.25, 5: 2.0}

    def set_lr(opt, k):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * factor[k]

    prev = torch.are_deterministic_algorithms_enabled()
    determinism.enable()
    try:
        m1, o1, s1, g1 = _graph_setup()
        assert m1.resolved_backend(cuda()) == "hip"
        eager = []
        for k in range(1, 6):
            if k in factor:
                set_lr(o1, k)
            eager.append(s1(*g1.next_batch()).item())
        m2, o2, s2, g2 = _graph_setup()
        gs = GraphedStep(s2, g2.next_batch, warmup=2)
        graphed = []
        for k in (3, 4, 5):
            set_lr(o2, k)
            graphed.append(gs().item())
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(prev)
        determinism._STATE["on"] = False
    assert eager[2:] == graphed, (eager, graphed)
    assert o1.step_count == o2.step_count == 5 and float(o2._step_dev.item()) == 5.0
    assert torch.equal(o1._hp_dev, o2._hp_dev)
    for x, y in ((o1.arena.data, o2.arena.data), (o1.exp_avg, o2.exp_avg), (o1.exp_avg_sq, o2.exp_avg_sq),
                 (o1.shadow, o2.shadow)):
        assert bits_equal(x, y)
    assert "pbx_adam_flat_groups" in _lib._FN


# ---- i: the session's launcher report -----------------------------------------------------------------------------
def test_launcher_report_lists_the_grouped_launcher():
    """tests/conftest.py reports the launchers reached through _lib.call (the keys of _lib._FN) at the end of
    a GPU session: the grouped launcher is exported, parsed from its prototype and reached."""
    assert "pbx_adam_flat_groups" in _lib.launchers() and len(_lib.launchers()["pbx_adam_flat_groups"]) == 13
    p, m, v = (guarded(np.ones(64, np.float32)) for _ in range(3))
    hps = torch.from_numpy(hp_blocks()).to(cuda())
    adam_groups(p, torch.ones(64, device=cuda()), m, v, None, 64, hps, 3, MASK, guarded(np.zeros(1, np.uint8), torch.uint8))
    torch.cuda.synchronize()
    assert "pbx_adam_flat_groups" in _lib._FN


if __name__ == "__main__":
    for gi_, rows in measure_table().items():
        print(f"    {gi_}: {{")
        for t_, e_ in rows.items():
            print(f"        {t_}: ({e_[0]:.3g}, {e_[1]:.3g}, {e_[2]:.3g}),")
        print("    },")
