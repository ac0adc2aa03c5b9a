"""GPU: the attention-map kernels (``pbx_attn_map_scores`` and ``pbx_attn_map_normalize``, csrc/attn_maps.hip)
alone, on random bf16 states, against an fp64 CPU oracle built from the same bf16 ``h2``, the bf16-rounded ``Wk``
and the kernel's own fp32 ``qs`` input.

``|kernel - fp64| <= 16 e + 2^-24`` for every element, ``e`` the worst absolute error over the case of an
independent fp32 torch evaluation of the same weights from the same operands (the bound of
tests/test_hip_score_heads.py, for the same reasons: 16 is the width granted to ``__expf`` and the MFMA
accumulation order).  ``qs`` as ``pbx_sg_query_fwd`` produces it is held to the same bound against fp64
``tanh(g Wq) / 8``.  Exactly: masked columns are ``+0.0``, all-masked rows are zero, nothing is written outside the
output or the partials, two launches agree bitwise, a sample's rows give the same bits at another batch index of a
larger batch, and block ``i`` of an 8-block launch gives the bits of a 1-block launch on that block.

Inputs: ``h2 = randn`` (bf16), ``Wk = randn * 128^-0.5``, ``g = randn``, ``Wq = randn * 2 G^-0.5``: the randn scale
of the model's own init saturates every ``tanh`` and would blind the test.  The condition that they do not is
asserted on the oracle: every row with at least 32 live positions has ``max p >= 1.5 mean p`` over its live
positions.  Masks: random tails plus interior zeros, one all-masked sequence where ``B > 1``; ``(2, 33)`` runs
with ``mask = None``.

The shapes: a lone position, a partial 32-position tile, one position past a tile, one past a 256-position chunk,
whole chunks, a ragged third chunk.  ``(40, 33)`` with 8 heads and 8 blocks has 320 (block, sample, chunk) items,
more than the launcher's grid cap for 8 heads, ``pbx_attn_map_grid_cap(8)`` = one workgroup per CU (256 on
MI355X; two per CU up to 4 heads): the grid-stride loop runs twice and a workgroup restages the key image."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, L, H, blocks, masked)
CASES = [(1, 1, 1, 1, True), (3, 31, 2, 2, True), (2, 33, 3, 1, False), (5, 257, 4, 8, True), (2, 512, 8, 2, True),
         (3, 600, 2, 8, True), (40, 33, 8, 8, True)]
G = 256
F64 = torch.float64
EPS = 2.0 ** -24
SENTINEL = -7.0
GUARD = 32
CHUNK = 256


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(*pairs):
    return all(bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + view.numel():] == SENTINEL).all())
               for buf, view in pairs)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _addr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _weights(p64, mask):
    """softmax over the live positions, by explicit max / exp / sum; zeros where masked or without one."""
    s = p64 if mask is None else p64.masked_fill(~mask[:, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    return torch.where(z > 0, e / z.clamp(min=1e-300), torch.zeros_like(e))


@functools.lru_cache(maxsize=None)
def _case(B, L, H, nb, masked):
    """Inputs on the GPU, the kernel's own operands (``qs``, key images) and the fp64 CPU oracle with the error
    ``e`` of an independent fp32 evaluation, computed once per case and only read."""
    from proteinbert_pytorch_replication_amd.ops import _lib
    gen = torch.Generator(device="cuda").manual_seed(1000 * B + L + H + nb)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)      # noqa: E731
    h2 = [rn(B, L, 128).to(torch.bfloat16) for _ in range(nb)]
    Wk = [rn(H, 128, 64) * 128 ** -0.5 for _ in range(nb)]
    g = [rn(B, G) for _ in range(nb)]
    Wq = [rn(H, G, 64) * 2 * G ** -0.5 for _ in range(nb)]
    mask = None
    if masked:
        n_live = torch.randint(1, L + 1, (B,), device="cuda", generator=gen)
        n_live[0] = L
        mask = torch.arange(L, device="cuda")[None, :] < n_live[:, None]
        mask &= torch.rand(B, L, device="cuda", generator=gen) > 0.1    # interior zeros
        mask[0, 0] = True
        if B > 1:
            mask[1] = False                                             # a sequence without a live position
        mask = mask.contiguous()
    st = _lib.stream_ptr(h2[0].device)
    ws = torch.empty(_lib.lib().pbx_sg_query_ws(B, G, H, 64), device="cuda")
    q = torch.empty(B, H, 64, device="cuda")
    qs = [torch.empty(B, H, 64, device="cuda") for _ in range(nb)]
    wimg = [torch.empty(H, 64, 128, dtype=torch.bfloat16, device="cuda") for _ in range(nb)]
    for i in range(nb):
        _lib.call("pbx_sg_query_fwd", g[i].data_ptr(), Wq[i].data_ptr(), q.data_ptr(), qs[i].data_ptr(), ws.data_ptr(),
                  B, G, H, 64, 0.125, st)
        _lib.call("pbx_pa_wimg", Wk[i].data_ptr(), Wk[i].data_ptr(), wimg[i].data_ptr(), H, 128, 64, 0, st)
    torch.cuda.synchronize()
    for i in range(nb):                          # the key image is the bf16 rounding of Wk, rows = key columns
        assert torch.equal(wimg[i], Wk[i].to(torch.bfloat16).transpose(1, 2))
    mk = None if mask is None else mask.cpu()
    ref, r32 = [], []
    for i in range(nb):
        hc, wc, qc = h2[i].cpu(), Wk[i].to(torch.bfloat16).cpu(), qs[i].cpu()
        a = torch.einsum("blc,hck->bhlk", hc.to(F64), wc.to(F64))
        ref.append(_weights(torch.einsum("bhk,bhlk->bhl", qc.to(F64), torch.tanh(a)), mk))
        a32 = torch.einsum("blc,hck->bhlk", hc.float(), wc.float())    # the independent fp32 evaluation
        s32 = torch.einsum("bhk,bhlk->bhl", qc, torch.tanh(a32))
        if mk is not None:
            s32 = s32.masked_fill(~mk[:, None, :], float("-inf"))
        r32.append(torch.nan_to_num(torch.softmax(s32, dim=-1), nan=0.0))
    ref, r32 = torch.stack(ref, 1), torch.stack(r32, 1)                  # [B, nb, H, L]
    e = float((r32.to(F64) - ref).abs().max())
    qref = [torch.tanh(torch.einsum("bg,hgk->bhk", g[i].cpu().to(F64), Wq[i].cpu().to(F64))) / 8 for i in range(nb)]
    q32 = [torch.tanh(torch.einsum("bg,hgk->bhk", g[i].cpu(), Wq[i].cpu())) / 8 for i in range(nb)]
    return dict(B=B, L=L, H=H, nb=nb, h2=h2, Wk=Wk, g=g, Wq=Wq, mask=mask, mk=mk, qs=qs, wimg=wimg, ref=ref, e=e,
                qref=qref, eq=max(float((a.to(F64) - b).abs().max()) for a, b in zip(q32, qref)))


def _launch(c, h2=None, qs=None, wimg=None, mask="case", blocks=None):
    """Both launchers on sentinel-guarded buffers: ``((out buffer, view), (partials buffer, view))``; ``blocks``:
    the block indices to run as one launch (default: all of the case)."""
    from proteinbert_pytorch_replication_amd.ops import _lib
    blocks = list(range(c["nb"])) if blocks is None else blocks
    h2 = [c["h2"][i] for i in blocks] if h2 is None else h2
    qs = [c["qs"][i] for i in blocks] if qs is None else qs
    wimg = [c["wimg"][i] for i in blocks] if wimg is None else wimg
    mask = c["mask"] if isinstance(mask, str) else mask
    B, L, _ = h2[0].shape
    H, n = c["H"], len(blocks)
    st = _lib.stream_ptr(h2[0].device)
    out = _guarded(B * n * H * L)
    part = _guarded(B * n * H * (-(-L // CHUNK)) * 2)
    _lib.call("pbx_attn_map_scores", _addr(h2), _addr(wimg), _addr(qs), _lib.ptr(mask), out[1].data_ptr(),
              part[1].data_ptr(), B, L, H, n, 0, n, st)
    _lib.call("pbx_attn_map_normalize", out[1].data_ptr(), part[1].data_ptr(), B, L, H, n, 0, n, st)
    return out, part


@functools.lru_cache(maxsize=None)
def _stored(*case):
    o = _launch(_case(*case))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("case", CASES)
def test_maps_against_fp64(case):
    c = _case(*case)
    B, L, H, nb = c["B"], c["L"], c["H"], c["nb"]
    out, part = _stored(*case)
    assert _guards_intact(out, part)
    got = out[1].cpu().view(B, nb, H, L)
    ref, e, mk = c["ref"], c["e"], c["mk"]
    # the condition on the inputs: the weights are far from uniform wherever a row has enough positions
    live = torch.ones(B, L, dtype=torch.bool) if mk is None else mk
    n = live.sum(1)
    ratio = ref.max(-1).values * n[:, None, None].clamp(min=1)           # max p / mean p over the live positions
    rows = n >= 32
    if rows.any():
        print(f"maps {case}: min max p / mean p over rows with >= 32 live positions {float(ratio[rows].min()):.2f}")
        assert float(ratio[rows].min()) >= 1.5
    err = (got.to(F64) - ref).abs()
    print(f"maps {case}: e {e:.3e} max err {float(err.max()):.3e} worst err / (16 e + 2^-24) "
          f"{float(err.max()) / (16 * e + EPS):.3f}")
    assert (err <= 16 * e + EPS).all()
    # exactly: masked columns +0.0, all-masked rows zero, live rows sum to 1
    if mk is not None:
        dead = got[~mk[:, None, None, :].expand_as(got)]
        assert (dead == 0).all() and not torch.signbit(dead).any()
        none = n == 0
        assert (got[none] == 0).all() and not torch.signbit(got[none]).any()
        if B > 1:
            assert bool(none[1])
    assert ((got.to(F64).sum(-1) - 1).abs()[n > 0] <= L * 2.0 ** -23).all()


@pytest.mark.parametrize("case", CASES)
def test_query_against_fp64(case):
    """``qs`` of ``pbx_sg_query_fwd``, the kernels' input, against fp64 ``tanh(g Wq) / 8``."""
    c = _case(*case)
    for i in range(c["nb"]):
        err = (c["qs"][i].cpu().to(F64) - c["qref"][i]).abs()
        assert (err <= 16 * c["eq"] + EPS).all(), i
    print(f"qs {case}: e {c['eq']:.3e} worst err / (16 e + 2^-24) "
          f"{max(float((c['qs'][i].cpu().to(F64) - c['qref'][i]).abs().max()) for i in range(c['nb'])) / (16 * c['eq'] + EPS):.3f}")


@pytest.mark.parametrize("case", CASES)
def test_exact_properties(case):
    from proteinbert_pytorch_replication_amd.data.vocab import PAD_ID
    from proteinbert_pytorch_replication_amd.ops.attention_maps import attention_maps, attention_supported, grid_cap
    c = _case(*case)
    B, L, H, nb = c["B"], c["L"], c["H"], c["nb"]
    out, part = _stored(*case)
    again = _launch(c)
    tokens = None if c["mask"] is None else torch.where(c["mask"], 5, PAD_ID)
    assert attention_supported(c["h2"], c["Wk"])
    api = attention_maps(c["h2"], c["g"], c["Wq"], c["Wk"], tokens)
    torch.cuda.synchronize()
    assert _guards_intact(*again)
    assert torch.equal(_bits(out[0]), _bits(again[0][0])) and torch.equal(_bits(part[0]), _bits(again[1][0]))
    assert api.shape == (B, nb, H, L) and api.dtype == torch.float32
    assert torch.equal(_bits(api).flatten(), _bits(out[1]))            # the Python entry: the same launches
    items = nb * B * (-(-L // CHUNK))
    cap = grid_cap(H)
    assert cap >= 1
    if case == CASES[-1]:
        assert items > cap                                              # the grid-stride loop ran
    if nb == 8:                                  # block i of the 8-block launch: the bits of a 1-block launch
        got = out[1].view(B, nb, H, L)
        for i in (0, 3, 7):
            one = _launch(c, blocks=[i])
            torch.cuda.synchronize()
            assert _guards_intact(*one)
            assert torch.equal(_bits(one[0][1].view(B, H, L)), _bits(got[:, i])), i


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4], CASES[5]])
def test_rows_do_not_depend_on_their_place_or_on_the_batch(case):
    """Sample ``s`` of the case as row 9 of a batch of 14 other samples: another batch size, grid and item
    index, the same bits."""
    c = _case(*case)
    B, L, H, nb = c["B"], c["L"], c["H"], c["nb"]
    out, _ = _stored(*case)
    s = 2 if B > 2 else 0
    gen = torch.Generator(device="cuda").manual_seed(11)
    h2, qs = [], []
    for i in range(nb):
        h = torch.randn(14, L, 128, device="cuda", generator=gen).to(torch.bfloat16)
        q = torch.randn(14, H, 64, device="cuda", generator=gen) * 0.1
        h[9], q[9] = c["h2"][i][s], c["qs"][i][s]
        h2.append(h)
        qs.append(q)
    mask = torch.rand(14, L, device="cuda", generator=gen) > 0.2
    mask[9] = c["mask"][s]
    moved = _launch(c, h2=h2, qs=qs, mask=mask.contiguous())
    torch.cuda.synchronize()
    assert _guards_intact(*moved)
    assert torch.equal(_bits(moved[0][1].view(14, nb, H, L)[9]), _bits(out[1].view(B, nb, H, L)[s]))


def test_more_than_eight_blocks_take_several_launches():
    from proteinbert_pytorch_replication_amd.ops.attention_maps import attention_maps
    c = _case(*CASES[1])
    order = [0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1]                           # 11 blocks: launches of 8 and 3
    pick = lambda k: [c[k][i] for i in order]                           # noqa: E731
    api = attention_maps(pick("h2"), pick("g"), pick("Wq"), pick("Wk"), None)
    base = attention_maps(c["h2"], c["g"], c["Wq"], c["Wk"], None)
    torch.cuda.synchronize()
    assert api.shape == (c["B"], 11, c["H"], c["L"])
    for j, i in enumerate(order):
        assert torch.equal(_bits(api[:, j]), _bits(base[:, i])), j


def test_out_of_limit_arguments_return_invalid_value_without_launching():
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.ops.attention_maps import attention_maps, attention_supported
    c = _case(*CASES[1])
    B, L, H = c["B"], c["L"], c["H"]
    st = _lib.stream_ptr(c["h2"][0].device)
    out, part = _guarded(B * 9 * 9 * L), _guarded(B * 9 * 9 * 2)
    nine = lambda k: _addr([c[k][0]] * 9)                               # noqa: E731
    good = [nine("h2"), nine("wimg"), nine("qs"), _lib.ptr(c["mask"]), out[1].data_ptr(), part[1].data_ptr(), B, L, H,
            2, 0, 2, st]
    for i, v in ((8, 9), (8, 0), (9, 9), (9, 0), (7, 0), (6, 0), (10, 1), (4, None), (5, None), (0, None)):
        args = list(good)
        args[i] = v
        if (i, v) == (9, 9):
            args[11] = 9                         # 9 blocks of a 9-block map: over the launch's limit of 8
        with pytest.raises(_lib.HipError, match="pbx_attn_map_scores failed"):
            _lib.call("pbx_attn_map_scores", *args)
    good = [out[1].data_ptr(), part[1].data_ptr(), B, L, H, 2, 0, 2, st]
    for i, v in ((4, 9), (4, 0), (5, 9), (5, 0), (3, 0), (2, 0), (6, 1), (0, None), (1, None)):
        args = list(good)
        args[i] = v
        if (i, v) == (5, 9):
            args[7] = 9
        with pytest.raises(_lib.HipError, match="pbx_attn_map_normalize failed"):
            _lib.call("pbx_attn_map_normalize", *args)
    torch.cuda.synchronize()
    assert bool((out[0] == SENTINEL).all()) and bool((part[0] == SENTINEL).all())
    assert {"pbx_attn_map_scores", "pbx_attn_map_normalize"} <= set(_lib._FN)
    # the Python entry: outside the kernel's range it raises before any launch
    calls = []
    real = _lib.call
    _lib.call = lambda *a: calls.append(a)
    try:
        bad9 = torch.randn(9, 128, 64, device="cuda")
        assert not attention_supported(c["h2"], [bad9] * 2)
        for kw in (dict(h2=[h.float() for h in c["h2"]]), dict(Wk=[bad9] * 2, Wq=[torch.randn(9, G, 64, device="cuda")] * 2),
                   dict(tokens=torch.zeros(B, L + 1, dtype=torch.long, device="cuda")), dict(g=c["g"][:1])):
            a = dict(h2=c["h2"], g=c["g"], Wq=c["Wq"], Wk=c["Wk"], tokens=None)
            a.update(kw)
            with pytest.raises(ValueError):
                attention_maps(a["h2"], a["g"], a["Wq"], a["Wk"], a["tokens"])
    finally:
        _lib.call = real
    assert not calls
