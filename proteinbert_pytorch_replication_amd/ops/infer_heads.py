"""Prediction heads for inference (``csrc/infer.hip``, ``csrc/score.hip``, ``EPI_GO_PROB`` in ``csrc/gemm.hip``).

The training heads produce a loss and gradients, the evaluation heads (:mod:`.eval_heads`) loss partials and
counts; neither returns a prediction.  Here each head writes what :mod:`..inference` hands to the caller:

* :func:`go_probs` -- the GO head as one MFMA GEMM launch whose epilogue stores ``sigmoid(z)`` (``z`` is never
  stored, no elementwise pass follows);
* :func:`row_topk` -- the ``k`` largest entries of every row, descending, equal values in ascending index
  order (``torch.sort(descending=True, stable=True)[:k]``), one wave per row with the row in registers;
* :func:`local_probs` -- the local head of either semantics: optional probabilities ``[B, L, V]``, the called
  token of every position (the lowest index of the maximum of the stored probabilities) and its probability;
* :func:`masked_mean_pool` -- the mean of ``h`` over the non-``<pad>`` positions;
* :func:`token_head_calls` -- a fine-tuned per-residue task head (``csrc/finetune.hip``): the class of every
  residue, its probability and optionally the class probabilities, from 1..8 row sources in one launch whose
  logits stay in registers;
* :func:`local_scores` -- variant-effect and likelihood scores from the local head's logits
  (``csrc/score.hip``): per-position log-odds of every substitution, the log-probability of the residue that
  is there and the entropy, and the per-sequence pseudo-log-likelihood, identical in both semantics
  (:func:`local_scores_torch` is the same definition on any device).

No autograd Function is involved, nothing is kept for a backward pass, and every output is bitwise repeatable.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib, finetune_head
from ..data.vocab import UNK_ID
from .finetune_head import MAX_SOURCES
from .global_track import bf16_of

F32 = torch.float32
TOPK_MAX_K = 64                 # pbx_row_topk: results live one per lane of a wave
TOPK_MAX_COLS = 256 * 64        # ... and the row in registers, at most 256 values per lane
SCORE_MAX_V = 32                # pbx_lhead_scores: the padded vocabulary of one MFMA tile


def _s(dev) -> int:
    return _lib.stream_ptr(dev)


def topk_supported(A: int, k: int) -> bool:
    """Whether :func:`row_topk` takes ``k`` of ``A`` columns (outside: ``torch.sort(..., stable=True)``)."""
    return 1 <= A <= TOPK_MAX_COLS and 1 <= k <= min(TOPK_MAX_K, A)


def go_probs(g_bf: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sigmoid(g_bf Wa^T + ba)`` as fp32 ``[B, A]`` (``pbx_go_head_probs``): operands as
    :func:`.eval_heads.go_head_eval` (``g_bf`` bf16, the bf16 mirror of ``Wa``).  ``out``: an fp32 ``[B, A]``
    tensor or view with unit column stride to write into (only its ``[B, A]`` elements are written)."""
    B, A = g_bf.shape[0], wa.shape[0]
    if out is None:
        out = torch.empty((B, A), dtype=F32, device=g_bf.device)
    if out.shape != (B, A) or out.dtype != F32 or out.stride(1) != 1 or out.stride(0) < A:
        raise ValueError(f"go_probs: out must be fp32 [{B}, {A}] with unit column stride")
    gx = g_bf.contiguous()
    wab = bf16_of(wa)
    _lib.call("pbx_go_head_probs", gx.data_ptr(), gx.stride(0), wab.data_ptr(), wab.stride(0),
              ba.detach().float().contiguous().data_ptr(), out.data_ptr(), out.stride(0), B, A, gx.shape[1],
              _s(g_bf.device))
    return out


def row_topk(P: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` largest entries of every row of ``P [B, A]`` fp32 (unit column stride, any row stride; finite
    values): ``(values [B, k] fp32, indices [B, k] int32)``, descending, ties by ascending index.  Raises
    ``ValueError`` outside :func:`topk_supported`, before any launch."""
    if P.dim() != 2 or P.dtype != F32:
        raise ValueError("row_topk: expected a 2-D fp32 matrix")
    B, A = P.shape
    if not topk_supported(A, k):
        raise ValueError(f"row_topk: k={k} of A={A} columns is outside the kernel's range "
                         f"(1 <= k <= min({TOPK_MAX_K}, A), A <= {TOPK_MAX_COLS})")
    if B < 1:
        raise ValueError("row_topk: empty matrix")
    if P.stride(1) != 1 or P.stride(0) < A:
        P = P.contiguous()
    val = torch.empty((B, k), dtype=F32, device=P.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=P.device)
    _lib.call("pbx_row_topk", P.data_ptr(), P.stride(0), B, A, int(k), val.data_ptr(), idx.data_ptr(), _s(P.device))
    return val, idx


def _probs_out(out: Optional[torch.Tensor], store_probs: bool, B: int, L: int, V: int,
               dev) -> Optional[torch.Tensor]:
    if not store_probs:
        return None
    if out is None:
        return torch.empty((B, L, V), dtype=F32, device=dev)
    if out.shape != (B, L, V) or out.dtype != F32 or not out.is_contiguous():
        raise ValueError(f"probabilities: out must be a contiguous fp32 [{B}, {L}, {V}] tensor")
    return out


def local_probs_ref(h: torch.Tensor, wo: torch.Tensor, bo: torch.Tensor, store_probs: bool = True,
                    out: Optional[torch.Tensor] = None):
    """Reference-semantics local head (softmax over the BATCH axis): stage A of the training head
    (``pbx_local_head3_a``: logits and the folded (M, 1/S) of every (position, token)) and one prediction pass.
    Returns ``(P [B, L, V] fp32 or None, tok [B, L] int32, pmax [B, L] fp32)``; ``out``: a contiguous fp32
    ``[B, L, V]`` tensor to write ``P`` into."""
    dev = h.device
    st = _s(dev)
    B, L, C = h.shape
    V = wo.shape[0]
    assert C == 128 and h.dtype == torch.bfloat16 and h.is_contiguous()
    P = _probs_out(out, store_probs, B, L, V, dev)
    nch = (B + 15) // 16
    Z = torch.empty((B * L, 32), dtype=F32, device=dev)
    part = torch.empty((nch, L, 32, 2), dtype=F32, device=dev)
    ms = torch.empty((L, 32, 2), dtype=F32, device=dev)
    _lib.call("pbx_local_head3_a", h.data_ptr(), wo.detach().float().contiguous().data_ptr(),
              bo.detach().float().contiguous().data_ptr(), Z.data_ptr(), part.data_ptr(), ms.data_ptr(),
              0, B, L, V, st)
    tok = torch.empty((B, L), dtype=torch.int32, device=dev)
    pmax = torch.empty((B, L), dtype=F32, device=dev)
    _lib.call("pbx_local_probs_ref", Z.data_ptr(), ms.data_ptr(), _lib.ptr(P), tok.data_ptr(), pmax.data_ptr(),
              int(store_probs), B, L, V, st)
    return P, tok, pmax


def local_probs_paper(h: torch.Tensor, wo: torch.Tensor, bo: torch.Tensor, store_probs: bool = True,
                      out: Optional[torch.Tensor] = None):
    """Paper-semantics local head (softmax over the vocabulary), one launch.  Returns as
    :func:`local_probs_ref`."""
    dev = h.device
    B, L, C = h.shape
    V = wo.shape[0]
    assert C == 128 and h.dtype == torch.bfloat16 and h.is_contiguous()
    P = _probs_out(out, store_probs, B, L, V, dev)
    tok = torch.empty((B, L), dtype=torch.int32, device=dev)
    pmax = torch.empty((B, L), dtype=F32, device=dev)
    _lib.call("pbx_phead_probs", h.data_ptr(), wo.detach().float().contiguous().data_ptr(),
              bo.detach().float().contiguous().data_ptr(), _lib.ptr(P), tok.data_ptr(), pmax.data_ptr(),
              int(store_probs), B * L, V, _s(dev))
    return P, tok, pmax


def local_probs(model, h: torch.Tensor, store_probs: bool = True):
    """The local head of ``model`` (by ``model.semantics``) on ``h [B, L, 128]`` bf16: ``(P or None, tok,
    pmax)``.  In reference semantics every output depends on the whole batch."""
    lo = model.pretraining_local_output[0]
    fn = local_probs_paper if model.semantics == "paper" else local_probs_ref
    return fn(h, lo.weight, lo.bias, store_probs)


def _task_head_args(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                    gterm: Optional[torch.Tensor], tokens: Optional[torch.Tensor]) -> Tuple[int, int, int]:
    """``(B, L, K)`` of a task-head call, or ``ValueError``: shapes only, so it holds on any device."""
    if not 1 <= len(hs) <= MAX_SOURCES:
        raise ValueError(f"token_head_calls: {len(hs)} row sources: expected 1 .. {MAX_SOURCES}")
    h0 = hs[0]
    if any(h.dim() != 3 or h.shape != h0.shape or h.device != h0.device or h.dtype != h0.dtype for h in hs):
        raise ValueError("token_head_calls: the sources must be [B, L, C] tensors of one shape, dtype and device")
    B, L, C = h0.shape
    if B < 1 or L < 1:
        raise ValueError("token_head_calls: empty sources")
    K = weight.shape[0] if weight.dim() == 2 else 0
    if not 1 <= K <= 16:
        raise ValueError(f"token_head_calls: weight {tuple(weight.shape)}: expected [K, {len(hs) * C}], 1 <= K <= 16")
    if weight.shape[1] != len(hs) * C:
        raise ValueError(f"token_head_calls: weight {tuple(weight.shape)} for {len(hs)} sources of {C} channels")
    if tuple(bias.shape) != (K,):
        raise ValueError(f"token_head_calls: bias {tuple(bias.shape)}: expected {(K,)}")
    if gterm is not None and tuple(gterm.shape) != (B, K):
        raise ValueError(f"token_head_calls: gterm {tuple(gterm.shape)}: expected {(B, K)}")
    if tokens is not None and (tuple(tokens.shape) != (B, L) or tokens.dtype != torch.int64):
        raise ValueError(f"token_head_calls: tokens must be int64 {(B, L)}")
    return B, L, K


def token_head_calls(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                     gterm: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None,
                     store_probs: bool = False, out: Optional[torch.Tensor] = None, min_token: int = UNK_ID):
    """Prediction with a per-residue task head (``pbx_token_head_calls``, one launch): ``hs``: 1..8 bf16
    ``[B, L, 128]`` row sources (the last block's state, or every block's for ``hidden="all"``), ``weight``
    ``[K, nb*128]``, ``bias`` ``[K]``, ``gterm`` ``[B, K]`` (the global term, added last), ``K <= 16``.  Returns
    ``(P [B, L, K] fp32 or None, labels [B, L] int32, pmax [B, L] fp32)``: the softmax over the classes of the
    logits :class:`.finetune_head.MultiTokenHeadFn` would store (they are never written), the lowest class of
    maximal stored probability and that probability.  With ``tokens`` ``[B, L]`` int64 a position whose token is
    below ``min_token`` (``<pad>``, ``<sos>``, ``<eos>``) gets label -1, probability 0 and a zero row.  ``out``: a
    contiguous fp32 ``[B, L, K]`` tensor to write ``P`` into.  Everything is validated before the launch."""
    B, L, K = _task_head_args(hs, weight, bias, gterm, tokens)
    if not finetune_head.supported_multi(hs, K):
        raise ValueError("token_head_calls: the sources must be CUDA bf16 [B, L, 128] tensors "
                         "(token_head_calls_torch is the definition on any device)")
    dev = hs[0].device
    P = _probs_out(out, store_probs, B, L, K, dev)
    rows = [finetune_head._rows(h) for h in hs]
    w32 = weight.detach().float().contiguous()
    b32 = bias.detach().float().contiguous()
    gt = None if gterm is None else gterm.detach().float().contiguous()
    tk = None if tokens is None else tokens.contiguous()
    labels = torch.empty((B, L), dtype=torch.int32, device=dev)
    pmax = torch.empty((B, L), dtype=F32, device=dev)
    _lib.call("pbx_token_head_calls", finetune_head._src_array(rows), len(rows), w32.data_ptr(), b32.data_ptr(),
              _lib.ptr(gt), _lib.ptr(tk), int(min_token), _lib.ptr(P), labels.data_ptr(), pmax.data_ptr(), B * L, K, L,
              _s(dev))
    return P, labels, pmax


def token_head_calls_torch(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                           gterm: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None,
                           store_probs: bool = False, out: Optional[torch.Tensor] = None, min_token: int = UNK_ID):
    """:func:`token_head_calls` by definition, on any device and for any channel count: fp32
    ``softmax(Linear(cat_i h_i) + gterm)`` over the classes, the first maximal index of the probabilities as
    computed (``argmax``), label -1 / zeros at the masked positions."""
    B, L, K = _task_head_args(hs, weight, bias, gterm, tokens)
    P = _probs_out(out, store_probs, B, L, K, hs[0].device)
    probs = torch.softmax(finetune_head.multi_head_torch(hs, weight.detach().float(), bias.detach().float(),
                                                         None if gterm is None else gterm.detach().float()), dim=-1)
    labels = probs.argmax(dim=-1)
    pmax = probs.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
    labels = labels.to(torch.int32)
    if tokens is not None:
        live = tokens >= min_token
        labels = torch.where(live, labels, torch.full_like(labels, -1))
        pmax = pmax * live
        probs = probs * live.unsqueeze(-1)
    if P is not None:
        P.copy_(probs)
    return P, labels, pmax


def _score_args(h: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, tokens: torch.Tensor,
                store_llr: bool, out: Optional[torch.Tensor]) -> Tuple[int, int, int]:
    """``(B, L, V)`` of a :func:`local_scores` call, or ``ValueError``: shapes and dtypes only, so it holds on
    any device."""
    if h.dim() != 3 or h.shape[0] < 1 or h.shape[1] < 1:
        raise ValueError(f"local_scores: h {tuple(h.shape)}: expected a non-empty [B, L, C] tensor")
    B, L, C = h.shape
    V = weight.shape[0] if weight.dim() == 2 else 0
    if not 1 <= V <= SCORE_MAX_V or weight.shape[1] != C:
        raise ValueError(f"local_scores: weight {tuple(weight.shape)}: expected [V, {C}], 1 <= V <= {SCORE_MAX_V}")
    if tuple(bias.shape) != (V,):
        raise ValueError(f"local_scores: bias {tuple(bias.shape)}: expected {(V,)}")
    if tuple(tokens.shape) != (B, L) or tokens.dtype != torch.int64:
        raise ValueError(f"local_scores: tokens must be int64 {(B, L)}")
    if out is not None and not store_llr:
        raise ValueError("local_scores: out= is where llr is stored: pass store_llr=True")
    if out is not None:
        _probs_out(out, True, B, L, V, None)        # its shape, dtype and layout
        if out.device != h.device:
            raise ValueError("local_scores: out must be on h's device")
    return B, L, V


def local_scores(h: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, tokens: torch.Tensor,
                 store_llr: bool = False, out: Optional[torch.Tensor] = None):
    """Scores from the local head's logits ``z = h bf16(W)^T + b`` (``pbx_lhead_scores`` and
    ``pbx_seq_score_fold``, ``csrc/score.hip``; the operands and accumulation of :func:`local_probs_paper`), the
    same in both semantics: ``h [B, L, 128]`` bf16, ``weight [V, 128]``, ``bias [V]``, ``V <= 32``, ``tokens
    [B, L]`` int64.  Returns ``(llr [B, L, V] fp32 or None, logp [B, L], entropy [B, L], pll [B] fp32, n_live
    [B] int32)``.  At a live position (``UNK_ID <= token < V``: not ``<pad>``, ``<sos>``, ``<eos>``, nor an id
    outside the vocabulary, which indexes nothing) ``llr[a] = z[a] - z[token]`` (the token's own column is
    ``+0.0``), ``logp = log softmax_v(z)[token]`` and ``entropy`` that of ``softmax_v(z)`` in nats; elsewhere
    zeros.  ``pll`` is the sum of the stored ``logp`` over the ``n_live`` live positions, accumulated in fp64
    in an order fixed by ``L`` and rounded once.  Every row's outputs depend on that row alone.  ``llr`` is
    written only with ``store_llr`` (``out``: a contiguous fp32 ``[B, L, V]`` tensor to write it into); without
    it the launch writes 8 bytes per row.  Everything is validated before the launch."""
    B, L, V = _score_args(h, weight, bias, tokens, store_llr, out)
    if not (h.is_cuda and h.dtype == torch.bfloat16 and h.shape[2] == 128):
        raise ValueError("local_scores: h must be a CUDA bf16 [B, L, 128] tensor "
                         "(local_scores_torch is the definition on any device)")
    if tokens.device != h.device:
        raise ValueError("local_scores: tokens must be on h's device")
    dev = h.device
    llr = _probs_out(out, store_llr, B, L, V, dev)
    hx = h.contiguous()
    tk = tokens.contiguous()
    logp = torch.empty((B, L), dtype=F32, device=dev)
    ent = torch.empty((B, L), dtype=F32, device=dev)
    pll = torch.empty((B,), dtype=F32, device=dev)
    n_live = torch.empty((B,), dtype=torch.int32, device=dev)
    st = _s(dev)
    _lib.call("pbx_lhead_scores", hx.data_ptr(), weight.detach().float().contiguous().data_ptr(),
              bias.detach().float().contiguous().data_ptr(), tk.data_ptr(), _lib.ptr(llr), logp.data_ptr(),
              ent.data_ptr(), int(store_llr), B * L, V, st)
    _lib.call("pbx_seq_score_fold", logp.data_ptr(), tk.data_ptr(), pll.data_ptr(), n_live.data_ptr(), B, L, V, st)
    return llr, logp, ent, pll, n_live


def local_scores_torch(h: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, tokens: torch.Tensor,
                       store_llr: bool = False, out: Optional[torch.Tensor] = None):
    """:func:`local_scores` by definition, on any device and for any channel count, in fp32: ``z =
    Linear(h.float())``, ``llr`` as a difference of logits, ``logp`` and ``entropy`` from ``log_softmax`` over
    the vocabulary, ``pll`` as the fp64 sum of the fp32 ``logp`` rounded once.  Each row is computed from that
    row alone, so a sequence's outputs do not change with its batch mates."""
    B, L, V = _score_args(h, weight, bias, tokens, store_llr, out)
    llr = _probs_out(out, store_llr, B, L, V, h.device)
    tokens = tokens.to(h.device)
    z = torch.nn.functional.linear(h.float(), weight.detach().float(), bias.detach().float())      # [B, L, V]
    live = (tokens >= UNK_ID) & (tokens < V)
    x = torch.where(live, tokens, torch.zeros_like(tokens)).unsqueeze(-1)       # a safe index where not live
    lq = torch.log_softmax(z, dim=-1)
    zero = torch.zeros((), dtype=F32, device=h.device)
    logp = torch.where(live, lq.gather(-1, x).squeeze(-1), zero)
    ent = torch.where(live, -(lq.exp() * lq).sum(-1), zero)
    if llr is not None:
        d = z - z.gather(-1, x)
        d.scatter_(-1, x, 0.0)                                                  # the token's own column: +0.0
        llr.copy_(torch.where(live.unsqueeze(-1), d, zero))
    pll = logp.to(torch.float64).sum(dim=1).to(F32)
    return llr, logp, ent, pll, live.sum(dim=1).to(torch.int32)


def masked_mean_pool(h: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """Mean of ``h [B, L, 128]`` bf16 over the positions with ``tokens [B, L] != 0`` (``<pad>``), fp32
    ``[B, 128]``, accumulated in fp32 in a fixed order; zeros for a sequence of pads only."""
    B, L, C = h.shape
    assert C == 128 and h.dtype == torch.bfloat16 and h.is_contiguous()
    if tokens.shape != (B, L) or tokens.dtype != torch.int64:
        raise ValueError("masked_mean_pool: tokens must be int64 [B, L]")
    out = torch.empty((B, C), dtype=F32, device=h.device)
    _lib.call("pbx_masked_mean_pool", h.data_ptr(), tokens.contiguous().data_ptr(), out.data_ptr(), B, L,
              _s(h.device))
    return out
