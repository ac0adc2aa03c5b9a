"""CPU: the host oracles of tests/step_oracles.py are right on their own, so the GPU tests of the data
kernels (test_hip_data_exact.py) need only bitwise equality and the Adam tolerances of
test_hip_optim_flat.py are known to separate a correct bias correction from an off-by-one.

Every seed is fixed, so each test is deterministic.  Rates are held to 5 binomial standard deviations,
uniformity to the chi-square critical value at 0.001 (df 63: 103.442, df 22: 48.268, df 21: 46.797).
"""
import numpy as np
import torch

import step_oracles as so
from proteinbert_pytorch_replication_amd.data.synthetic import CorruptionParams, corrupt_batch_torch

CHI2_999 = {63: 103.442, 22: 48.268, 21: 46.797}
DEFAULTS = dict(token_p=0.05, positive_p=0.25, negative_p=1e-4, blank_p=0.5)


def chi2_uniform(counts):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def assert_rate(k, n, p, what):
    sd = np.sqrt(n * p * (1.0 - p))
    assert abs(k - n * p) <= 5.0 * sd, (what, k, n, k / n, p)


def corrupt(tok, ann, seed, step=1, **kw):
    q = dict(DEFAULTS, **kw)
    return so.corrupt_batch_ref(tok, ann, q["token_p"], q["positive_p"], q["negative_p"], q["blank_p"], seed, step)


def test_golden_hash_values():
    """Cross-checked between a host C++ copy of common.h's pbx_mix64 / pbx_uniform and this numpy replica."""
    assert int(so.uniform_bits(0, 1, 0)[0]) == 10009755
    assert int(so.uniform_bits(7, 21, 255)[0]) == 11134291
    assert int(so.uniform_bits(2 ** 64 - 1, 16000057, 8589934597)[0]) == 6762464
    assert so.uniform(7, 21, 255)[0] == np.float32(11134291 / 16777216)
    assert so.stream_id(2 ** 32 + 3, so.S_AA) == (2 ** 32 + 3) * 16 + 3
    assert so.stream_id(2 ** 64 - 1, so.S_LEN, step_dev=2) == 17          # wraps modulo 2^64


def test_uniform_range_and_histogram():
    u = so.uniform(11, so.stream_id(5, so.S_ANN), np.arange(1 << 20))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    counts = np.bincount((u * np.float32(64)).astype(np.int64), minlength=64)
    assert chi2_uniform(counts) < CHI2_999[63]


def test_token_corruption_rate_range_and_specials():
    B, L = 1024, 1100                                   # B * L = 1,126,400 draws
    tok, _ = so.synth_batch_ref(B, L, 1, 0, L + 64, 0.0, seed=3, step=1)
    tok[:, 5][tok[:, 5] > so.EOS] = 3                   # id 3 is eligible for corruption
    ann = np.zeros((B, 1), np.float32)
    x, _, w_local, _ = corrupt(tok, ann, seed=3)
    special = tok <= so.EOS
    assert np.array_equal(x[special], tok[special])
    assert np.array_equal(w_local, (tok != so.PAD).astype(np.float32))
    eligible = int((~special).sum())
    assert eligible >= 1 << 19
    # a replacement is drawn from {3..25} and equals the old id with probability 1/23
    assert_rate(int((x != tok).sum()), eligible, 0.05 * 22 / 23, "token corruption")
    # token_p = 1: every eligible id is replaced, specials never; the replacements are uniform on {3..25}
    x1, _, _, _ = corrupt(tok, ann, seed=3, token_p=1.0)
    assert np.array_equal(x1[special], tok[special])
    rep = x1[~special]
    assert rep.min() == 3 and rep.max() == 25
    assert chi2_uniform(np.bincount(rep, minlength=26)[3:]) < CHI2_999[22]
    # and the mask rate itself, read off the token_p = 1 replacements: x == x1 wherever the mask fired
    fired = (x == x1) & ~special & (x1 != tok)
    assert_rate(int(fired.sum()), int(((x1 != tok) & ~special).sum()), 0.05, "token mask")
    x0, _, _, _ = corrupt(tok, ann, seed=3, token_p=0.0)
    assert np.array_equal(x0, tok)


def test_annotation_corruption_rates():
    B, A = 128, 8943                                    # B * A = 1,144,704 draws
    tok = np.full((B, 4), 7, np.int64)
    ones, zeros = np.ones((B, A), np.float32), np.zeros((B, A), np.float32)
    # keep: blank_p = 0 (u <= 0 only for u == 0), negative_p = 0, so out = keep
    _, xg, _, ws = corrupt(tok, ones, seed=5, blank_p=0.0, negative_p=0.0)
    assert set(np.unique(xg)) <= {0.0, 1.0} and np.all(ws == 1.0)
    assert_rate(int(xg.sum()), B * A, 0.75, "keep")
    # add: positive_p = 0 keeps everything, so out = add
    _, xg, _, ws = corrupt(tok, zeros, seed=5, blank_p=0.0, positive_p=0.0)
    assert np.all(ws == 0.0)
    assert_rate(int(xg.sum()), B * A, float(np.float32(1e-4)), "add")
    # both: (ann + add) * keep is 2.0 where an added annotation meets a present one
    _, xg, _, _ = corrupt(tok, ones, seed=5, blank_p=0.0, negative_p=1.0, positive_p=0.0)
    assert np.all(xg == 2.0)
    # blank: one row per draw; blank_p = 1 blanks every row
    B2 = 1 << 20
    tok2, one2 = np.full((B2, 1), 7, np.int64), np.ones((B2, 1), np.float32)
    _, xg, _, _ = corrupt(tok2, one2, seed=5, positive_p=0.0, negative_p=0.0)
    assert_rate(int((xg[:, 0] == 0).sum()), B2, 0.5, "blank")
    _, xg, _, _ = corrupt(tok, ones, seed=5, blank_p=1.0)
    assert not xg.any()


def test_synth_density_and_residues():
    B, L, A = 129, 8192, 8943
    density = 0.005
    tok, ann = so.synth_batch_ref(B, L, A, L - 2, L - 2, density, seed=9, step=2)
    assert tok.dtype == np.int64 and ann.dtype == np.float32
    assert set(np.unique(ann)) <= {0.0, 1.0}
    assert_rate(int(ann.sum()), B * A, float(np.float32(density)), "annotation density")
    assert np.all(tok[:, 0] == so.SOS) and np.all(tok[:, -1] == so.EOS)
    res = tok[:, 1:-1].ravel()
    assert res.size >= 1 << 20 and res.min() == 4 and res.max() == 25
    assert chi2_uniform(np.bincount(res, minlength=26)[4:]) < CHI2_999[21]


def test_synth_rows_structure():
    """Lengths cover [min_len, max_len]; rows are <sos> aa.. <eos> <pad>.. when uncropped."""
    B, L = 4096, 40
    n, start = so.synth_rows_ref(B, L, 0, 30, seed=1, step=1)
    assert set(np.unique(n)) == set(range(31)) and not start.any()
    tok, _ = so.synth_batch_ref(B, L, 3, 0, 30, 0.5, seed=1, step=1)
    pos = np.arange(L)[None, :]
    assert np.all(tok[:, 0] == so.SOS)
    assert np.all(tok[pos == (n + 1)[:, None]] == so.EOS)
    assert np.all(tok[pos > (n + 1)[:, None]] == so.PAD)
    inner = (pos > 0) & (pos <= n[:, None])
    assert np.all(tok[inner] >= 4) and np.all(tok[inner] <= 25)
    # min_len = 0 reaches the row <sos><eos><pad>...
    assert np.any((tok[:, 1] == so.EOS) & (tok[:, 2:] == so.PAD).all(axis=1))


def test_crop_start_is_exclusive():
    """With max_len + 2 > L the start takes every value in [0, total - L - 1] and never total - L."""
    B, L, n_res = 4096, 50, 60                          # total = 62, span = 12
    n, start = so.synth_rows_ref(B, L, n_res, n_res, seed=2, step=1)
    total = n_res + 2
    assert np.all(n == n_res)
    assert set(np.unique(start)) == set(range(total - L))
    tok, _ = so.synth_batch_ref(B, L, 1, n_res, n_res, 0.0, seed=2, step=1)
    assert np.array_equal(tok[:, 0] == so.SOS, start == 0)
    assert not (tok == so.EOS).any() and not (tok == so.PAD).any()   # the quirk: <eos> is never in the window
    # span 1: the start must be 0
    _, start1 = so.synth_rows_ref(B, L, L - 1, L - 1, seed=2, step=1)
    assert not start1.any()


def test_corrupt_ref_matches_torch_on_deterministic_outputs():
    B, L, A = 33, 300, 517
    tok, ann = so.synth_batch_ref(B, L, A, 0, L + 64, 0.002, seed=4, step=1)
    ann[0] = 0
    ann[1] = 0
    ann[1, A - 1] = 1
    _, _, w_local, w_sample = corrupt(tok, ann, seed=4)
    _, Y, W = corrupt_batch_torch(torch.from_numpy(tok), torch.from_numpy(ann), CorruptionParams(),
                                  torch.Generator().manual_seed(0))
    assert torch.equal(Y["local"], torch.from_numpy(tok)) and torch.equal(Y["global"], torch.from_numpy(ann))
    assert torch.equal(W["local"], torch.from_numpy(w_local))
    assert torch.equal(W["global"], torch.from_numpy(w_sample)[:, None].expand(B, A))
    assert w_sample[0] == 0 and w_sample[1] == 1


def test_unpack_ref():
    bits = np.array([[0b10000001, 0xFF], [0b00000010, 0x00]], np.uint8)
    tok, ann = so.unpack_ref(np.array([[0, 255], [3, 7]], np.uint8), bits, 9)
    assert tok.dtype == np.int64 and tok.tolist() == [[0, 255], [3, 7]]
    assert ann.tolist() == [[1, 0, 0, 0, 0, 0, 0, 1, 1], [0, 1, 0, 0, 0, 0, 0, 0, 0]]


def test_adam_oracles_agree_with_torch():
    """adam_ref64 is torch.optim.Adam (float64) with the gradient scaled first."""
    rng = np.random.default_rng(0)
    n = 1000
    p0, hp = so.adam_p0(n), so.adam_hp()
    q = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([q], lr=float(hp[0]), betas=(float(hp[1]), float(hp[2])), eps=float(hp[3]),
                           weight_decay=float(hp[4]))
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        q.grad = torch.from_numpy(g).double() * float(hp[7])
        opt.step()
        p, m, v = so.adam_ref64(p, g, m, v, hp, t)
        np.testing.assert_allclose(p, q.detach().numpy(), rtol=1e-12, atol=1e-15)
    # the host path takes hp[5], hp[6] as given
    hp2 = so.hp_block(1e-2, 0.9, 0.999, 1e-8, 0.0, bc1=0.37, bc2_sqrt=1.7)
    p2, _, _ = so.adam_ref64(np.zeros(1), np.ones(1), np.zeros(1), np.zeros(1), hp2)
    m1, v1 = 1.0 - float(hp2[1]), 1.0 - float(hp2[2])
    assert np.isclose(p2[0], -(float(hp2[0]) / float(hp2[5])) * m1 / (np.sqrt(v1) / float(hp2[6]) + float(hp2[3])),
                      rtol=1e-14)


def test_adam_tolerance_separates_off_by_one():
    """The comparison the GPU test makes, with adam_emul32 standing in for the kernel, at t = 1, 2, 3, 10 and
    at the GPU test's t = 11..13 (non-zero moments): with the right t it is inside ADAM_EMUL_TABLE (so inside
    the 4x bound); with bias corrections from t + 1 the parameter error exceeds the 4x bound at every step."""
    n = 1 << 17
    good, bad = {}, {}
    for steps in ((1, 2, 3, 10), (1, 2, 3, 11, 12, 13)):
        good.update(so.measure_adam_table(n, steps=steps))
        bad.update(so.measure_adam_table(n, steps=steps, t_shift=1))
    for t in sorted(good):
        tab = so.ADAM_EMUL_TABLE[t]
        print(t, "emulation", good[t], "table", tab, "off-by-one", bad[t])
        assert all(e <= x for e, x in zip(good[t], tab)), (t, good[t], tab)
        assert bad[t][0] > so.ADAM_KERNEL_FACTOR * tab[0], (t, bad[t], tab)
        # the moments do not depend on the bias correction
        assert bad[t][1:] == good[t][1:]
    # the separation is wide: the off-by-one costs 0.26 of a step at t = 1 and still 4e-3 at t = 10,
    # against an emulation error of 4e-6 at the most
    assert bad[1][0] > 0.2 and bad[10][0] > 1e-3
