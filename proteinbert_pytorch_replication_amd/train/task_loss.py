"""The training loss of per-residue tasks: cross-entropy with class weights and label smoothing.

Residue tasks are imbalanced (DSSP-8 has classes under 2 % of the residues), and macro-F1 or per-class recall,
which :mod:`.evaluate_finetune` reports and ``finetune(select_metric=...)`` selects by, move only when the rare
classes weigh more in the objective.  :class:`ResidueTaskLoss` is that objective.  With ``p = softmax(z)``,
``w`` the class weights (ones when none are given), ``S = sum_k w_k`` and ``eps`` the smoothing, a live row
contributes

    loss_row = (1 - eps) * w_y * (-log p_y) + (eps / K) * sum_k w_k * (-log p_k)

and the loss is ``sum loss_row / sum w_y`` over the live rows: ``F.cross_entropy(z, y, weight=w,
ignore_index=..., label_smoothing=eps)``.  Its gradient with respect to a live row's logits is

    (1 - eps) * w_y * (p_k - [k == y]) + (eps / K) * (p_k * S - w_k),       divided by sum w_y.

Called as ``loss_fn(logits [B, K, L], y [B, L])`` it is that torch expression, on any device and for any model.
Given to :func:`.finetune.train_step` with a :class:`..models.finetune.ProteinBERTForTokenClassification` on a
GPU, the step takes the model's fused form instead (``model.loss``: one HIP launch for logits, loss, accuracy
and the logit gradient, :class:`..ops.finetune_head.TokenHeadLossFn`).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import torch
import torch.nn.functional as F

# counter() layout
N_LIVE, N_HITS, N_BAD = 0, 1, 2


def _device(device) -> torch.device:
    """``device`` with its index spelled out (``cuda`` is the current ``cuda:i``): one key per physical device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class ResidueTaskLoss(torch.nn.Module):
    """``ResidueTaskLoss(class_weights=None, label_smoothing=0.0, ignore_index=-100)``.

    ``class_weights``: ``[K]`` floats (a tensor or a sequence), or ``None`` for an unweighted loss;
    :func:`balanced_class_weights` derives them from the training labels.  ``label_smoothing``: ``0 <= eps < 1``.
    A batch without a live position has a ``nan`` loss and a zero gradient, as in torch."""

    def __init__(self, class_weights: Union[None, torch.Tensor, Sequence[float]] = None,
                 label_smoothing: float = 0.0, ignore_index: int = -100):
        super().__init__()
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise ValueError(f"label_smoothing={label_smoothing}: expected 0 <= eps < 1")
        cw = None
        if class_weights is not None:
            cw = torch.as_tensor(class_weights, dtype=torch.float32).detach().clone()
            if cw.dim() != 1 or cw.numel() < 1 or not bool(torch.isfinite(cw).all()) or bool((cw < 0).any()):
                raise ValueError("class_weights: expected a non-empty 1-D list of finite, non-negative weights")
        self.register_buffer("class_weights", cw)
        self.label_smoothing = eps
        self.ignore_index = int(ignore_index)
        self._cw: Dict[torch.device, torch.Tensor] = {}
        self._counter: Dict[torch.device, torch.Tensor] = {}

    def weights_on(self, device) -> Optional[torch.Tensor]:
        """The class weights on ``device`` (copied there once), or ``None``."""
        if self.class_weights is None:
            return None
        device = _device(device)
        if self.class_weights.device == device:
            return self.class_weights
        w = self._cw.get(device)
        if w is None:
            w = self._cw[device] = self.class_weights.to(device)
        return w

    def counter(self, device) -> torch.Tensor:
        """int64 ``[3]`` on ``device``: live rows, hits and labels ``>= K`` that ``model.loss`` has seen since
        the counter was last zeroed.  :func:`.finetune.train_step` zeroes it per epoch and reads it once."""
        device = _device(device)
        c = self._counter.get(device)
        if c is None:
            c = self._counter[device] = torch.zeros(3, dtype=torch.int64, device=device)
        return c

    def forward(self, logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        w = self.weights_on(logits.device)
        if w is not None and w.numel() != logits.shape[1]:
            raise ValueError(f"{w.numel()} class weights for logits of {logits.shape[1]} classes")
        return F.cross_entropy(logits, y, weight=w, ignore_index=self.ignore_index,
                               label_smoothing=self.label_smoothing)

    def extra_repr(self) -> str:
        cw = None if self.class_weights is None else [round(float(v), 6) for v in self.class_weights]
        return f"class_weights={cw}, label_smoothing={self.label_smoothing}, ignore_index={self.ignore_index}"


def balanced_class_weights(labels, n_classes: int, ignore_index: int = -100) -> torch.Tensor:
    """``n_live / (n_classes * count_k)`` per class, fp32 ``[n_classes]``: the weights under which every class
    that occurs contributes the same total weight, and an unweighted, perfectly balanced label set gets ones.
    A class that never occurs gets weight 0.  ``labels``: a tensor of any shape, or an iterable of tensors (for
    instance the label batches of a data loader); positions equal to ``ignore_index`` or negative are skipped,
    a label ``>= n_classes`` is an error.

    By hand, ``n_classes=4`` and labels ``[0, 0, 0, 0, 0, 0, 1, 1, 1, 3, -100, -100]``: ten live labels with
    counts ``[6, 3, 0, 1]``, so the weights are ``10 / (4 * 6) = 0.41667``, ``10 / (4 * 3) = 0.83333``, ``0``
    (class 2 is absent) and ``10 / (4 * 1) = 2.5``; each present class then carries ``count_k * w_k = 2.5``."""
    if n_classes < 1:
        raise ValueError(f"n_classes={n_classes}")
    counts = torch.zeros(n_classes, dtype=torch.int64)
    for t in ([labels] if isinstance(labels, torch.Tensor) else labels):
        t = torch.as_tensor(t).reshape(-1).to("cpu", torch.int64)
        t = t[(t != ignore_index) & (t >= 0)]
        if t.numel() and int(t.max()) >= n_classes:
            raise ValueError(f"label {int(t.max())} is outside 0..{n_classes - 1} (n_classes={n_classes})")
        counts += torch.bincount(t, minlength=n_classes)
    n_live = int(counts.sum())
    w = torch.zeros(n_classes, dtype=torch.float64)
    present = counts > 0
    w[present] = n_live / (n_classes * counts[present].double())
    return w.float()
