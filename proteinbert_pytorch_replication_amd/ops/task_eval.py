"""Evaluation of fine-tuned classification heads (``pbx_token_head_eval`` / ``pbx_task_eval_fold`` in
``csrc/finetune.hip``).

The training forward of a per-residue head writes the fp32 ``[B*L, K]`` logits, and the reference's ``test_step``
reads them three more times (cross-entropy, softmax, argmax) for one accuracy per batch.  Here a batch is one
launch with the staging of :func:`.infer_heads.token_head_calls`: the logits stay in registers, and a workgroup
writes the sum of its live rows' cross-entropy and a ``K x K`` confusion table (true x predicted).  One fold
launch per batch adds the partials, in a fixed order, into a :class:`TaskEvalAccumulator` on the device (an fp64
loss sum, int64 counts): an evaluation over many batches needs no host sync and cannot overflow, and accuracy,
per-class precision / recall / F1, macro- and weighted F1 and MCC all follow from the one table
(:func:`metrics_from_confusion`).

Row classes by the label: ``y < 0`` (the ``-100`` of the loaders) is ignored, ``0 <= y < K`` is live, ``y >= K``
is a bad label: counted, kept out of the table and the loss, and an error when the metrics are formed.  The call
of a live row is :func:`.infer_heads.token_head_calls`'s: the lowest class of maximal probability.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib, finetune_head
from .finetune_head import MAX_SOURCES

F32 = torch.float32
# TaskEvalAccumulator.counts layout after the K * K confusion entries (csrc/finetune.hip task_eval_fold_kernel)
C_LIVE, C_BAD, C_BATCHES, C_SEQS = 0, 1, 2, 3
N_EXTRA = 4


class TaskEvalAccumulator:
    """Persistent sums of an evaluation: ``loss`` fp64 [1] (the live rows' cross-entropy, summed), ``counts``
    int64 [K*K + 4]: the confusion matrix row-major true x predicted, then live rows, bad labels, batches and
    sequences."""

    def __init__(self, n_classes: int, device):
        if n_classes < 1:
            raise ValueError(f"TaskEvalAccumulator: n_classes={n_classes}")
        self.n_classes = int(n_classes)
        self.loss = torch.zeros(1, dtype=torch.float64, device=device)
        self.counts = torch.zeros(self.n_classes ** 2 + N_EXTRA, dtype=torch.int64, device=device)

    def zero_(self) -> "TaskEvalAccumulator":
        self.loss.zero_()
        self.counts.zero_()
        return self

    @property
    def confusion(self) -> torch.Tensor:
        K = self.n_classes
        return self.counts[:K * K].view(K, K)


def eval_parts(M: int) -> int:
    """Workgroups (= partial rows) of ``pbx_token_head_eval`` on ``M`` rows: workgroup ``w`` owns rows
    ``256 w .. 256 w + 255`` (the library's own answer: ``(M + 255) // 256``)."""
    return int(_lib.lib().pbx_token_head_eval_parts(int(M)))


def _eval_args(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
               gterm: Optional[torch.Tensor], y: torch.Tensor, acc: TaskEvalAccumulator) -> Tuple[int, int, int]:
    """``(B, L, K)`` of an evaluation call, or ``ValueError``: shapes, dtypes and devices, on any device."""
    if not 1 <= len(hs) <= MAX_SOURCES:
        raise ValueError(f"token_head_eval: {len(hs)} row sources: expected 1 .. {MAX_SOURCES}")
    h0 = hs[0]
    if any(h.dim() != 3 or h.shape != h0.shape or h.device != h0.device or h.dtype != h0.dtype for h in hs):
        raise ValueError("token_head_eval: the sources must be [B, L, C] tensors of one shape, dtype and device")
    B, L, C = h0.shape
    if B < 1 or L < 1:
        raise ValueError("token_head_eval: empty sources")
    K = weight.shape[0] if weight.dim() == 2 else 0
    if K < 1:
        raise ValueError(f"token_head_eval: weight {tuple(weight.shape)}: expected [K, {len(hs) * C}]")
    if weight.shape[1] != len(hs) * C:
        raise ValueError(f"token_head_eval: weight {tuple(weight.shape)} for {len(hs)} sources of {C} channels")
    if tuple(bias.shape) != (K,):
        raise ValueError(f"token_head_eval: bias {tuple(bias.shape)}: expected {(K,)}")
    if gterm is not None and tuple(gterm.shape) != (B, K):
        raise ValueError(f"token_head_eval: gterm {tuple(gterm.shape)}: expected {(B, K)}")
    if tuple(y.shape) != (B, L) or y.dtype != torch.int64:
        raise ValueError(f"token_head_eval: y must be int64 {(B, L)}")
    if acc.n_classes != K:
        raise ValueError(f"token_head_eval: an accumulator of {acc.n_classes} classes for a head of {K}")
    others = [weight, bias, y, acc.loss, acc.counts] + ([] if gterm is None else [gterm])
    if any(t.device != h0.device for t in others):
        raise ValueError("token_head_eval: sources, head, labels and accumulator must be on one device")
    return B, L, K


def token_head_eval(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                    gterm: Optional[torch.Tensor], y: torch.Tensor, acc: TaskEvalAccumulator) -> None:
    """One batch of a per-residue head into ``acc`` on the HIP path: ``pbx_token_head_eval`` (operands as
    :func:`.infer_heads.token_head_calls`; ``y`` ``[B, L]`` int64 labels) and ``pbx_task_eval_fold``, two launches
    on the current stream, no host sync.  Everything is validated before the first launch; sources outside
    :func:`.finetune_head.supported_multi` raise (:func:`token_head_eval_torch` is the definition anywhere)."""
    B, L, K = _eval_args(hs, weight, bias, gterm, y, acc)
    if not finetune_head.supported_multi(hs, K):
        raise ValueError("token_head_eval: the sources must be CUDA bf16 [B, L, 128] tensors and K <= 16 "
                         "(token_head_eval_torch is the definition on any device)")
    dev = hs[0].device
    M = B * L
    rows = [finetune_head._rows(h) for h in hs]
    w32 = weight.detach().float().contiguous()
    b32 = bias.detach().float().contiguous()
    gt = None if gterm is None else gterm.detach().float().contiguous()
    yc = y.contiguous()
    nwg = eval_parts(M)
    lparts = torch.empty(nwg, dtype=F32, device=dev)
    cparts = torch.empty((nwg, K * K + 2), dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.call("pbx_token_head_eval", finetune_head._src_array(rows), len(rows), w32.data_ptr(), b32.data_ptr(),
              _lib.ptr(gt), yc.data_ptr(), lparts.data_ptr(), cparts.data_ptr(), M, K, L, st)
    _lib.call("pbx_task_eval_fold", lparts.data_ptr(), cparts.data_ptr(), nwg, K, B, acc.loss.data_ptr(),
              acc.counts.data_ptr(), st)


def _bincount(idx: torch.Tensor, n: int) -> torch.Tensor:
    """Counts of the values ``0 .. n-1`` (``bincount``; sort + searchsorted where deterministic algorithms are
    demanded of a GPU, as in ``train.evaluate._hist``)."""
    if idx.is_cuda and torch.are_deterministic_algorithms_enabled():
        s = idx.reshape(-1).sort().values
        edges = torch.searchsorted(s, torch.arange(n + 1, device=s.device))
        return edges[1:] - edges[:-1]
    return torch.bincount(idx.reshape(-1), minlength=n)


def class_counts_into(acc: TaskEvalAccumulator, logits: torch.Tensor, y: torch.Tensor,
                      n_sequences: Optional[int] = None) -> None:
    """One batch from ready fp32 logits ``[N, K]`` and labels ``y [N]`` into ``acc``, in torch, with no host
    sync: the call ``softmax(logits).argmax(-1)``, the loss ``F.cross_entropy(reduction="sum")`` over the live
    rows, the confusion by ``bincount``.  Serves the per-protein heads (a few KB per batch) and is the body of
    :func:`token_head_eval_torch`.  ``n_sequences``: what the sequence counter advances by (default ``N``)."""
    K = acc.n_classes
    if logits.dim() != 2 or logits.shape[1] != K or tuple(y.shape) != (logits.shape[0],):
        raise ValueError(f"class_counts_into: logits {tuple(logits.shape)} / y {tuple(y.shape)}: expected "
                         f"[N, {K}] and [N]")
    z = logits.detach().float()
    y = y.to(torch.int64)
    live = (y >= 0) & (y < K)
    call = torch.softmax(z, dim=-1).argmax(dim=-1)
    ys = torch.where(live, y, torch.zeros_like(y))
    ce = F.cross_entropy(z, ys, reduction="none")
    acc.loss += (ce * live).sum().double()
    # dead rows go to an extra bin past the table
    idx = torch.where(live, ys * K + call, torch.full_like(ys, K * K))
    extra = torch.stack([live.sum(), (y >= K).sum(), torch.ones_like(live.sum()),
                         torch.full_like(live.sum(), logits.shape[0] if n_sequences is None else int(n_sequences))])
    acc.counts += torch.cat([_bincount(idx, K * K + 1)[:K * K], extra])


def token_head_eval_torch(hs: Sequence[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                          gterm: Optional[torch.Tensor], y: torch.Tensor, acc: TaskEvalAccumulator) -> None:
    """:func:`token_head_eval` by definition, on any device and for any channel and class count: the logits of
    :func:`.finetune_head.multi_head_torch`, then :func:`class_counts_into`."""
    B, L, K = _eval_args(hs, weight, bias, gterm, y, acc)
    z = finetune_head.multi_head_torch(hs, weight.detach().float(), bias.detach().float(),
                                       None if gterm is None else gterm.detach().float())
    class_counts_into(acc, z.reshape(B * L, K), y.reshape(-1), n_sequences=B)


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else float("nan")


def metrics_from_confusion(acc) -> Dict[str, Any]:
    """The metrics of an evaluation, from one read of ``acc`` (a :class:`TaskEvalAccumulator`, or anything with
    its ``n_classes`` / ``loss`` / ``counts``), on the host in fp64 and Python integers:

    ``n`` (live rows), ``loss`` (sum / n), ``accuracy``; per class (lists of K) ``precision``, ``recall``,
    ``f1``, ``support`` (true rows) and ``predicted`` (called rows); ``macro_f1`` (mean F1 over the classes that
    occur in the labels or the predictions), ``weighted_f1`` (by support), ``mcc`` (the multi-class coefficient
    of Gorodkin), ``confusion`` (nested list, true x predicted), ``n_batches``, ``n_sequences``.  A ratio with an
    empty denominator is ``nan``; an F1 with no true positive but a non-empty denominator is 0; ``mcc`` is ``nan``
    when its denominator is 0.  A non-zero bad-label count raises ``ValueError``."""
    K = int(acc.n_classes)
    dev = acc.counts.device
    # the one host read: both tensors in one copy (the fp64 sum travels as its bit pattern)
    host = torch.cat([acc.loss.view(torch.int64), acc.counts]).cpu() if dev.type != "cpu" else None
    loss_sum = float(acc.loss[0]) if host is None else float(host[:1].view(torch.float64)[0])
    c = [int(v) for v in (acc.counts if host is None else host[1:]).tolist()]
    cm = [c[t * K:(t + 1) * K] for t in range(K)]
    n, bad, nbatch, nseq = (c[K * K + i] for i in (C_LIVE, C_BAD, C_BATCHES, C_SEQS))
    if bad:
        raise ValueError(f"{bad} labels are outside 0..{K - 1} (n_classes={K}); labels below 0 are ignored")
    support = [sum(cm[t]) for t in range(K)]
    predicted = [sum(cm[t][p] for t in range(K)) for p in range(K)]
    tp = [cm[k][k] for k in range(K)]
    precision = [_ratio(tp[k], predicted[k]) for k in range(K)]
    recall = [_ratio(tp[k], support[k]) for k in range(K)]
    f1 = [_ratio(2 * tp[k], support[k] + predicted[k]) for k in range(K)]
    present = [k for k in range(K) if support[k] + predicted[k] > 0]
    total = sum(support)
    correct = sum(tp)
    # Gorodkin's R_K on integers: (c s - sum_k p_k t_k) / sqrt((s^2 - sum p_k^2) (s^2 - sum t_k^2))
    num = correct * total - sum(p * t for p, t in zip(predicted, support))
    den = (total * total - sum(p * p for p in predicted)) * (total * total - sum(t * t for t in support))
    return {
        "n": n, "loss": _ratio(loss_sum, n), "accuracy": _ratio(correct, total),
        "precision": precision, "recall": recall, "f1": f1, "support": support, "predicted": predicted,
        "macro_f1": _ratio(sum(f1[k] for k in present), len(present)),
        "weighted_f1": _ratio(sum(f1[k] * support[k] for k in range(K) if support[k]), total),
        "mcc": num / math.sqrt(den) if den > 0 else float("nan"),
        "confusion": cm, "n_batches": nbatch, "n_sequences": nseq,
    }


def scalar_metrics(m: Dict[str, Any]) -> Dict[str, Any]:
    """The scalar entries of a metrics dict (what logs and JSONL take): no lists, no tensors."""
    return {k: v for k, v in m.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
