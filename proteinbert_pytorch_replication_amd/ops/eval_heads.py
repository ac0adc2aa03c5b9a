"""Gradient-free pretraining heads for held-out evaluation (``csrc/evalhead.hip``, ``EPI_GO_EVAL`` in
``csrc/gemm.hip``).

The training heads (:class:`.global_track.HeadsLossFn`, :class:`.paper_track.PaperHeadsLossFn`) compute
the loss together with ``dh`` / ``dz``; an evaluation needs neither.  Here each head writes per-tile
partials only -- the loss, and what the metrics are made of:

* local head (either semantics): the number of positions with weight > 0, the hits (``argmax_v P == y``,
  lowest index on ties) among them, the number of *corrupted* positions among them (input token ``x`` !=
  target ``y``) and the hits among those;
* GO head: two 256-bin histograms of the predicted probability (``y = 1`` / ``y = 0``) over the entries
  with weight > 0 -- precision / recall / F1 at 0.5 and a binned AUROC follow from them.

One fold launch per batch adds the partials, in a fixed order, into an :class:`EvalAccumulator` on the
device (fp64 loss sums, int64 counts and histograms): an evaluation over many batches needs no host sync
and cannot overflow.  No autograd Function is involved and nothing is kept for a backward pass.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib, streams
from .gemm import go_head_parts
from .global_track import bf16_of
from ..parallel import batch_softmax

F32 = torch.float32
NBIN = 256                      # histogram bins of the GO probability per class
# EvalAccumulator.counts layout (csrc/evalhead.hip eval_fold_kernel)
C_BATCHES, C_SEQS, C_TOK, C_TOK_HIT, C_MASKED, C_MASKED_HIT = 0, 1, 2, 3, 4, 5
C_HIST = 8                      # hist(y = 1) [256], then hist(y = 0) [256]
N_COUNTS = C_HIST + 2 * NBIN


class EvalAccumulator:
    """Persistent sums of an evaluation: ``loss`` fp64 [2] (the batches' local / GO loss), ``counts`` int64
    [520] (batches, sequences, weighted / hit / corrupted / corrupted-and-hit positions, 2 reserved, the two
    GO histograms)."""

    def __init__(self, device):
        self.loss = torch.zeros(2, dtype=torch.float64, device=device)
        self.counts = torch.zeros(N_COUNTS, dtype=torch.int64, device=device)

    def zero_(self) -> "EvalAccumulator":
        self.loss.zero_()
        self.counts.zero_()
        return self

    @property
    def hist_pos(self) -> torch.Tensor:
        return self.counts[C_HIST:C_HIST + NBIN]

    @property
    def hist_neg(self) -> torch.Tensor:
        return self.counts[C_HIST + NBIN:C_HIST + 2 * NBIN]


def _s(dev) -> int:
    return _lib.stream_ptr(dev)


def local_head_eval(h: torch.Tensor, wo: torch.Tensor, bo: torch.Tensor, x_l: torch.Tensor, y_l: torch.Tensor,
                    w_l: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference-semantics local head (softmax over the batch axis): stage A of the training head
    (``pbx_local_head3_a``: logits and the folded (M, 1/S) of every (position, token)) and one evaluation
    pass.  With a shared batch softmax (:mod:`..parallel.batch_softmax`) the statistics are merged over the
    ranks between the two launches, as the training head does.  Returns (loss partials [tiles] fp32, each
    already divided by B L; counts [tiles, 4] int32)."""
    dev = h.device
    st = _s(dev)
    B, L, C = h.shape
    V = wo.shape[0]
    assert C == 128 and h.dtype == torch.bfloat16 and h.is_contiguous()
    nt = _lib.lib().pbx_local_head3_tiles(B, L)
    nch = (B + 15) // 16
    Z = torch.empty((B * L, 32), dtype=F32, device=dev)
    part = torch.empty((nch, L, 32, 2), dtype=F32, device=dev)
    ms = torch.empty((L, 32, 2), dtype=F32, device=dev)
    shared = batch_softmax.active()
    _lib.call("pbx_local_head3_a", h.data_ptr(), wo.detach().float().contiguous().data_ptr(),
              bo.detach().float().contiguous().data_ptr(), Z.data_ptr(), part.data_ptr(), ms.data_ptr(),
              int(shared), B, L, V, st)
    if shared:
        batch_softmax.merge_head_stats(ms)
    lparts = torch.empty(nt, dtype=F32, device=dev)
    cparts = torch.empty((nt, 4), dtype=torch.int32, device=dev)
    _lib.call("pbx_local_head_eval", Z.data_ptr(), ms.data_ptr(), y_l.contiguous().data_ptr(),
              x_l.contiguous().data_ptr(), w_l.float().contiguous().data_ptr(), lparts.data_ptr(), cparts.data_ptr(),
              B, L, V, st)
    return lparts, cparts


def paper_head_eval(h: torch.Tensor, wo: torch.Tensor, bo: torch.Tensor, x_l: torch.Tensor, y_l: torch.Tensor,
                    w_l: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Paper-semantics local head (softmax over the vocabulary, NLL), one launch.  Returns (loss partials
    [parts] fp32, each already divided by B L; counts [parts, 4] int32)."""
    dev = h.device
    B, L, C = h.shape
    V = wo.shape[0]
    assert C == 128 and h.dtype == torch.bfloat16 and h.is_contiguous()
    R = B * L
    parts = _lib.lib().pbx_phead_eval_parts(R)
    lparts = torch.empty(parts, dtype=F32, device=dev)
    cparts = torch.empty((parts, 4), dtype=torch.int32, device=dev)
    _lib.call("pbx_phead_eval", h.data_ptr(), wo.detach().float().contiguous().data_ptr(),
              bo.detach().float().contiguous().data_ptr(), y_l.reshape(-1).contiguous().data_ptr(),
              x_l.reshape(-1).contiguous().data_ptr(), w_l.reshape(-1).float().contiguous().data_ptr(),
              lparts.data_ptr(), cparts.data_ptr(), R, V, 1.0 / float(R), _s(dev))
    return lparts, cparts


def go_head_eval(g_bf: torch.Tensor, wa: torch.Tensor, ba: torch.Tensor, y_g: torch.Tensor,
                 w_g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """GO head as one MFMA GEMM launch with the evaluation epilogue (``pbx_go_head_eval``).  ``w_g``: per-row
    weights broadcast over the annotations (a stride-0 expand, read without expanding) or a full [B, A]
    tensor.  Returns (loss partials [tiles] fp32, each already divided by B A; histograms [tiles, 2, 256]
    int32: y = 1, then y = 0)."""
    dev = g_bf.device
    B, A = g_bf.shape[0], wa.shape[0]
    nt = go_head_parts(B, A)
    lparts = torch.empty(nt, dtype=F32, device=dev)
    hparts = torch.empty((nt, 2, NBIN), dtype=torch.int32, device=dev)
    y = y_g.float().contiguous()
    if w_g.dim() == 2 and w_g.stride(1) == 0:
        wrow, wfull = w_g[:, 0].float().contiguous(), None
    else:
        wrow, wfull = None, w_g.float().expand(B, A).contiguous()
    gx = g_bf.contiguous()
    wab = bf16_of(wa)
    _lib.call("pbx_go_head_eval", gx.data_ptr(), gx.stride(0), wab.data_ptr(), wab.stride(0),
              ba.detach().float().contiguous().data_ptr(), y.data_ptr(), A, _lib.ptr(wrow), _lib.ptr(wfull),
              lparts.data_ptr(), hparts.data_ptr(), B, A, gx.shape[1], _s(dev))
    return lparts, hparts


def fold(acc: EvalAccumulator, local_parts, go_parts, n_sequences: int) -> None:
    """Add one batch's partials into ``acc`` (one launch, fixed summation order)."""
    (ll, lc), (gl, gh) = local_parts, go_parts
    _lib.call("pbx_eval_fold", ll.data_ptr(), lc.data_ptr(), ll.numel(), gl.data_ptr(), gh.data_ptr(), gl.numel(),
              acc.loss.data_ptr(), acc.counts.data_ptr(), int(n_sequences), _s(acc.loss.device))


def eval_heads(model, h: torch.Tensor, g: torch.Tensor, g_bf: torch.Tensor, X_local: torch.Tensor,
               Y: Dict[str, torch.Tensor], W: Dict[str, torch.Tensor], acc: EvalAccumulator) -> None:
    """Both heads of ``model`` on the encoder outputs ``h [B, L, 128]`` bf16 / ``g_bf [B, G]`` bf16 (``g``,
    the fp32 global vector, is unused: the GO GEMM reads the bf16 copy, as in training), their losses and
    counts added into ``acc``.  Launches on the current stream; the GO head runs beside the local head on
    the "head" aux stream when aux streams are on."""
    dev = h.device
    lo, go = model.pretraining_local_output[0], model.pretraining_global_output[0]
    local = paper_head_eval if model.semantics == "paper" else local_head_eval
    y_g, w_g = Y["global"], W["global"]
    if streams.ENABLED and dev.type == "cuda":
        res = []

        def go_fn():
            res.append(go_head_eval(g_bf, go.weight, go.bias, y_g, w_g))
            return list(res[0])

        streams.launch(dev, go_fn, keep=[g_bf, y_g, w_g], name="head")
        lparts = local(h, lo.weight, lo.bias, X_local, Y["local"], W["local"])
        streams.wait_for(dev, "head")
        fold(acc, lparts, res[0], h.shape[0])
        streams.join()                      # releases the tensors kept for the aux stream
    else:
        gparts = go_head_eval(g_bf, go.weight, go.bias, y_g, w_g)
        lparts = local(h, lo.weight, lo.bias, X_local, Y["local"], W["local"])
        fold(acc, lparts, gparts, h.shape[0])
