"""GPU: the score kernels (``pbx_lhead_scores`` and ``pbx_seq_score_fold``, csrc/score.hip) alone, on random bf16
encoder outputs built as tests/test_hip_infer_heads.py::_case builds them, against an fp64 CPU oracle from the
same bf16 ``h`` and the bf16-rounded ``Wo``.

``llr``, ``logp``, ``entropy``: ``|kernel - fp64| <= 16 e + 2^-24`` for every element, ``e`` the worst absolute
error over the case of an independent fp32 torch evaluation of the same quantity from the same operands (16 is
the width tests/test_hip_infer_heads.py grants ``__expf`` and the MFMA accumulation order).  ``pll``: against the
fp64 sum ``s`` of the kernel's own stored ``logp`` over the live positions, ``|pll - s| <= (L - 1) 2^-53
sum|logp| + 2^-24 |s|`` (the summation bound of any order of L fp64 additions, plus one rounding to fp32).
``n_live``: exact.  Exactly: the wild-type column is +0.0, rows that are not live are zero, a launch without the
``llr`` store gives bitwise the same ``logp`` / ``entropy`` / ``pll`` and writes nothing to ``llr``, nothing is
written outside any output, two launches agree bitwise, and a sequence's rows give the same bits at another
batch index of a larger batch.

Tokens are uniform over ``[0, V)`` (every wild-type column, every special), with one all-``<pad>`` sequence and
ids outside ``[0, V)`` where the shape has room.  ``(257, 512)`` has 4112 row tiles, more than the 4096 one
trip of the capped grid (1024 workgroups of 4 waves) covers: the grid-stride loop runs."""
import functools

import pytest
import torch

from proteinbert_pytorch_replication_amd.data.vocab import PAD_ID, UNK_ID
from proteinbert_pytorch_replication_amd.models import ProteinBERT

pytestmark = pytest.mark.gpu

SHAPES = [(6, 24), (17, 33), (130, 37), (1, 1), (3, 512), (257, 512)]
CASES = [(B, L, 26) for B, L in SHAPES] + [(17, 33, 32), (17, 33, 5)]
F64 = torch.float64
EPS = 2.0 ** -24
SENTINEL = -7.0
GUARD = 32                      # sentinel elements on either side of every output


@functools.lru_cache(maxsize=None)
def _case(B, L, V):
    """Inputs on the GPU and the fp64 CPU oracle with the error ``e`` of an independent fp32 evaluation of
    every quantity, computed once per case and only read."""
    torch.manual_seed(B + L)
    m = ProteinBERT(sequences_length=L, num_annotations=96, local_dim=128, global_dim=256, key_dim=64, num_heads=4,
                    num_blocks=1, vocab_size=V, device="cuda", backend="hip")
    h = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    tokens = torch.randint(0, V, (B, L), device="cuda")
    if B >= 3:
        tokens[1] = PAD_ID                                        # a sequence without a live position
        tokens[B - 1, L - 1] = V                                  # ids outside [0, V): never an index
        tokens[0, 0], tokens[2, L // 2] = -3, 2 ** 40 + 5
    lo = m.pretraining_local_output[0]
    w32 = lo.weight.detach().float().contiguous()
    b32 = lo.bias.detach().float().contiguous()
    c = dict(B=B, L=L, V=V, h=h, tokens=tokens, lo=lo, w32=w32, b32=b32)
    tk = tokens.cpu()
    live = (tk >= UNK_ID) & (tk < V)
    x = torch.where(live, tk, torch.zeros_like(tk)).unsqueeze(-1)
    wo = lo.weight.detach().to(torch.bfloat16).cpu()
    bo = lo.bias.detach().cpu()

    def quantities(Z):
        lq = torch.log_softmax(Z, dim=-1)
        llr = (Z - Z.gather(-1, x)) * live.unsqueeze(-1)
        return dict(llr=llr, logp=lq.gather(-1, x).squeeze(-1) * live, entropy=-(lq.exp() * lq).sum(-1) * live)

    ref = quantities(h.cpu().to(F64) @ wo.to(F64).t() + bo.to(F64))
    r32 = quantities(h.cpu().float() @ wo.float().t() + bo)         # the independent fp32 evaluation
    c.update(live=live, x=x, ref=ref, e={k: float((r32[k].to(F64) - ref[k]).abs().max()) for k in ref})
    return c


def _guarded(n, dtype=torch.float32):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _launch(c, store_llr, h=None, tokens=None):
    """Both launchers on sentinel-guarded buffers: ``{name: (whole buffer, the output's view)}``."""
    from proteinbert_pytorch_replication_amd.ops import _lib
    h = c["h"] if h is None else h
    tokens = c["tokens"] if tokens is None else tokens
    B, L = tokens.shape
    V = c["V"]
    st = _lib.stream_ptr(h.device)
    o = dict(llr=_guarded(B * L * V), logp=_guarded(B * L), entropy=_guarded(B * L), pll=_guarded(B),
             n_live=_guarded(B, torch.int32))
    _lib.call("pbx_lhead_scores", h.data_ptr(), c["w32"].data_ptr(), c["b32"].data_ptr(), tokens.data_ptr(),
              o["llr"][1].data_ptr(), o["logp"][1].data_ptr(), o["entropy"][1].data_ptr(), int(store_llr), B * L, V, st)
    _lib.call("pbx_seq_score_fold", o["logp"][1].data_ptr(), tokens.data_ptr(), o["pll"][1].data_ptr(),
              o["n_live"][1].data_ptr(), B, L, V, st)
    return o


def _guards_intact(o):
    return all(bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + view.numel():] == SENTINEL).all())
               for buf, view in o.values())


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _stored(B, L, V):
    """One launch with the ``llr`` store, shared by the tests of a case and only read."""
    o = _launch(_case(B, L, V), True)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("B,L,V", CASES)
def test_scores_against_fp64(B, L, V):
    c = _case(B, L, V)
    o = _stored(B, L, V)
    assert _guards_intact(o)
    got = dict(llr=o["llr"][1].cpu().view(B, L, V), logp=o["logp"][1].cpu().view(B, L),
               entropy=o["entropy"][1].cpu().view(B, L))
    for name in ("llr", "logp", "entropy"):
        err = (got[name].to(F64) - c["ref"][name]).abs()
        e = c["e"][name]
        print(f"scores B={B} L={L} V={V} {name}: e {e:.3e} max err {float(err.max()):.3e} "
              f"worst err / e {float(err.max()) / max(e, 1e-300):.2f}")
    for name in ("llr", "logp", "entropy"):
        assert ((got[name].to(F64) - c["ref"][name]).abs() <= 16 * c["e"][name] + EPS).all(), name
    live = c["live"]
    lp64 = got["logp"].to(F64) * live
    s = lp64.sum(1)
    pll = o["pll"][1].cpu()
    bound = (L - 1) * 2.0 ** -53 * lp64.abs().sum(1) + EPS * s.abs()
    print(f"scores B={B} L={L} V={V} pll: worst err / bound "
          f"{float(((pll.to(F64) - s).abs() / bound.clamp(min=1e-300)).max()):.3f}")
    assert ((pll.to(F64) - s).abs() <= bound).all()
    assert torch.equal(o["n_live"][1].cpu().long(), live.sum(1))


@pytest.mark.parametrize("B,L,V", CASES)
def test_exact_properties(B, L, V):
    from proteinbert_pytorch_replication_amd.ops.infer_heads import local_scores
    c = _case(B, L, V)
    o = _stored(B, L, V)
    again = _launch(c, True)
    plain = _launch(c, False)                                    # llr points at a buffer that must stay untouched
    out = torch.empty((B, L, V), device="cuda")
    api = local_scores(c["h"], c["lo"].weight, c["lo"].bias, c["tokens"], store_llr=True, out=out)
    api_plain = local_scores(c["h"], c["lo"].weight, c["lo"].bias, c["tokens"])
    torch.cuda.synchronize()
    assert _guards_intact(again) and _guards_intact(plain)
    for name in o:                                               # two launches: the same bits
        assert torch.equal(_bits(o[name][0]), _bits(again[name][0])), name
    assert bool((plain["llr"][0] == SENTINEL).all())             # no store: nothing written to llr
    for name in ("logp", "entropy", "pll", "n_live"):            # ... and the same bits elsewhere
        assert torch.equal(_bits(o[name][1]), _bits(plain[name][1])), name
    # the Python entry: the same launches
    assert api[0].data_ptr() == out.data_ptr() and api_plain[0] is None
    assert api[4].dtype == torch.int32 and api[1].shape == (B, L) and api[3].shape == (B,)
    for res in (api, api_plain):
        for t, name in zip(res[1:], ("logp", "entropy", "pll", "n_live")):
            assert torch.equal(_bits(t).flatten(), _bits(o[name][1])), name
    assert torch.equal(_bits(api[0]).flatten(), _bits(o["llr"][1]))
    # the wild-type column is +0.0; a row that is not live is +0.0 everywhere
    live, x = c["live"], c["x"]
    llr = o["llr"][1].cpu().view(B, L, V)
    wt = llr.gather(-1, x).squeeze(-1)
    assert (wt == 0).all() and not torch.signbit(wt).any()
    dead = ~live
    for t in (llr[dead], o["logp"][1].cpu().view(B, L)[dead], o["entropy"][1].cpu().view(B, L)[dead]):
        assert (t == 0).all() and not torch.signbit(t).any()
    none_live = live.sum(1) == 0
    assert (o["pll"][1].cpu()[none_live] == 0).all() and (o["n_live"][1].cpu()[none_live] == 0).all()
    if B >= 3:
        assert bool(none_live[1]) and not live[B - 1, L - 1] and not live[0, 0] and not live[2, L // 2]


@pytest.mark.parametrize("B,L,V", [(6, 24, 26), (17, 33, 26), (3, 512, 26), (17, 33, 5)])
def test_rows_do_not_depend_on_their_place_or_on_the_batch(B, L, V):
    """Sequence ``s`` of the case as row 9 of a batch of 14 other sequences: another batch size, grid and place
    in the 32-row tiles (9 L rows further on), the same bits, ``pll`` included."""
    c = _case(B, L, V)
    o = _stored(B, L, V)
    s = B - 1 if B < 3 else 2
    gen = torch.Generator(device="cuda").manual_seed(11)
    h2 = torch.randn(14, L, 128, device="cuda", generator=gen).to(torch.bfloat16)
    t2 = torch.randint(0, V, (14, L), device="cuda", generator=gen)
    h2[9], t2[9] = c["h"][s], c["tokens"][s]
    moved = _launch(c, True, h2, t2)
    torch.cuda.synchronize()
    assert _guards_intact(moved)
    for name, width in (("llr", L * V), ("logp", L), ("entropy", L), ("pll", 1), ("n_live", 1)):
        a = o[name][1][s * width:(s + 1) * width]
        b = moved[name][1][9 * width:10 * width]
        assert torch.equal(_bits(a), _bits(b)), name


def test_argument_errors_raise_before_any_launch():
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.ops.infer_heads import local_scores
    c = _case(6, 24, 26)
    h, tokens, w, b = c["h"], c["tokens"], c["lo"].weight, c["lo"].bias
    calls = []
    real = _lib.call
    _lib.call = lambda *a: calls.append(a)      # any launch attempt would be recorded
    try:
        bad = [dict(h=h.float()), dict(h=h[..., :64].contiguous(), w=w[:, :64]), dict(tokens=tokens.int()),
               dict(tokens=tokens[:, :5]), dict(tokens=tokens.cpu()), dict(w=torch.zeros(33, 128, device="cuda"),
                                                                           b=torch.zeros(33, device="cuda")),
               dict(b=b[:7]), dict(h=h[:0], tokens=tokens[:0]), dict(out=torch.empty(6, 24, 27, device="cuda")),
               dict(out=torch.empty(6, 24, 26, device="cuda", dtype=torch.float64)),
               dict(out=torch.empty(6, 24, 26)), dict(out=torch.empty(6, 24, 26, device="cuda"), store_llr=False)]
        for kw in bad:
            a = dict(h=h, w=w, b=b, tokens=tokens, store_llr=True, out=None)
            a.update(kw)
            with pytest.raises(ValueError):
                local_scores(a["h"], a["w"], a["b"], a["tokens"], store_llr=a["store_llr"], out=a["out"])
    finally:
        _lib.call = real
    assert not calls
    # the launchers themselves: hipErrorInvalidValue and nothing written
    o = {k: _guarded(n, torch.int32 if k == "n_live" else torch.float32)
         for k, n in (("llr", 6 * 24 * 26), ("logp", 6 * 24), ("entropy", 6 * 24), ("pll", 6), ("n_live", 6))}
    st = _lib.stream_ptr(h.device)
    p = {k: v[1].data_ptr() for k, v in o.items()}
    good = [h.data_ptr(), c["w32"].data_ptr(), c["b32"].data_ptr(), tokens.data_ptr(), p["llr"], p["logp"],
            p["entropy"], 1, 6 * 24, 26, st]
    for i, v in ((9, 0), (9, 33), (8, 0), (0, None), (3, None), (4, None), (5, None), (6, None)):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.HipError, match="pbx_lhead_scores failed"):
            _lib.call("pbx_lhead_scores", *args)
    good = [p["logp"], tokens.data_ptr(), p["pll"], p["n_live"], 6, 24, 26, st]
    for i, v in ((4, 0), (5, 0), (6, 0), (6, 33), (0, None), (1, None), (2, None), (3, None)):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.HipError, match="pbx_seq_score_fold failed"):
            _lib.call("pbx_seq_score_fold", *args)
    torch.cuda.synchronize()
    assert all(bool((buf == SENTINEL).all()) for buf, _ in o.values())
    assert {"pbx_lhead_scores", "pbx_seq_score_fold"} <= set(_lib._FN)
