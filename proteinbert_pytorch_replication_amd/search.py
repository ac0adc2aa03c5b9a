"""Similarity search over protein embeddings: an index of embedded proteins and exact top-k neighbours.

    index = EmbeddingIndex.from_sequences(pred, db_seqs, ids=db_ids, embedding="global", metric="cosine")
    index.add(more_vectors, ids=more_ids)                  # rows keep insertion order
    hits = index.search_sequences(pred, query_seqs, k=10)  # or index.search(vectors [Q, D], k=10)
    hits["indices"], hits["scores"], hits["ids"]           # [Q, k] int64 / fp32 / list of lists, input order
    index.save("db.npz"); index = EmbeddingIndex.load("db.npz", device="cuda")

**Score.**  The stored rows and the queries are bf16; ``score[q, r] = sum_d float(Q[q, d]) * float(X[r, d])``,
accumulated in fp32.  ``metric="cosine"``: rows and queries are divided by their Euclidean norm in fp32 and then
rounded to bf16 (a zero vector is an error); ``metric="dot"``: they are only rounded to bf16.

**Order.**  Hits are the first ``k`` rows of the total order (score descending, then row index ascending): equal
scores come back in insertion order, and two runs return the same neighbours.

On a GPU the search is one fused launch per query batch (:func:`.ops.search.search_topk`: the ``[Q, N]`` score
matrix is never stored) whenever :func:`.ops.search.search_supported` takes the shape; on the CPU, or for a
dimension that is no multiple of 16, above 1024, or ``k > 64``, it is :func:`.ops.search.search_topk_torch`, the
same definition in chunks.  ``embedding`` is ``"global"`` or ``"pooled"`` (:mod:`.inference`): neither depends on
the sequences sharing a batch, in either semantics, so an index does not depend on how it was batched.

**File.**  ``save`` writes an ``.npz`` with ``rows`` (the bf16 matrix as ``uint16`` ``[N, D]``), ``ids`` and
``meta``, a JSON string with ``metric``, ``embedding``, ``dim`` and ``version``.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .ops import search as _ops

METRICS = ("cosine", "dot")
EMBEDDINGS = ("global", "pooled")
FORMAT_VERSION = 1
MAX_SCORE_ELEMENTS = 2 ** 31


class EmbeddingIndex:
    """Embedded proteins as a bf16 matrix ``[N, dim]`` on ``device``, searched exactly (module docstring).
    ``embedding`` names what the rows are (``"global"``, ``"pooled"`` or None for vectors of any origin)."""

    def __init__(self, dim: int, metric: str = "cosine", embedding: Optional[str] = None, device="cpu"):
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: expected one of {METRICS}")
        if embedding is not None and embedding not in EMBEDDINGS:
            raise ValueError(f"embedding {embedding!r}: expected one of {EMBEDDINGS}")
        if dim < 1:
            raise ValueError("dim must be positive")
        self.dim = int(dim)
        self.metric = metric
        self.embedding = embedding
        self.device = torch.device(device)
        self.ids: List[str] = []
        self._chunks: List[torch.Tensor] = []       # bf16 [n_i, dim] on self.device, in insertion order
        self._matrix: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return len(self.ids)

    # ------------------------------------------------------------------------
    def _rows(self, vectors: torch.Tensor, what: str) -> torch.Tensor:
        """``vectors [M, dim]`` as the bf16 rows the metric compares, on the index's device."""
        v = torch.as_tensor(vectors)
        if v.dim() != 2 or v.shape[1] != self.dim:
            raise ValueError(f"{what}: expected [M, {self.dim}] vectors, got {tuple(v.shape)}")
        v = v.detach().to(self.device).float()
        if not bool(torch.isfinite(v).all()):
            raise ValueError(f"{what}: non-finite values")
        if self.metric == "cosine":
            norm = v.norm(dim=1, keepdim=True)
            if bool((norm == 0).any()):
                raise ValueError(f"{what}: a zero vector has no direction (metric='cosine')")
            v = v / norm
        return v.to(torch.bfloat16)

    def add(self, vectors: torch.Tensor, ids: Optional[Sequence[str]] = None) -> None:
        """Append ``vectors [M, dim]`` (any float dtype, any device); ``ids``: one name per row (default: the
        row numbers as strings).  Rows keep insertion order."""
        rows = self._rows(vectors, "add")
        m = rows.shape[0]
        if ids is None:
            ids = [str(len(self.ids) + i) for i in range(m)]
        ids = [str(i) for i in ids]
        if len(ids) != m:
            raise ValueError(f"add: {len(ids)} ids for {m} vectors")
        if m == 0:
            return
        if len(self.ids) + m > _ops.MAX_N:
            raise ValueError(f"an index holds at most {_ops.MAX_N} rows")
        self._chunks.append(rows)
        self.ids.extend(ids)
        self._matrix = None

    @property
    def matrix(self) -> torch.Tensor:
        """The stored rows, bf16 ``[N, dim]``: built once from the added pieces."""
        if self._matrix is None:
            if not self._chunks:
                return torch.empty((0, self.dim), dtype=torch.bfloat16, device=self.device)
            self._matrix = self._chunks[0] if len(self._chunks) == 1 else torch.cat(self._chunks, dim=0)
            self._chunks = [self._matrix]
        return self._matrix

    def _fused(self, k: int) -> bool:
        return self.device.type == "cuda" and _ops.search_supported(self.dim, k, len(self))

    # ------------------------------------------------------------------------
    def search(self, vectors: torch.Tensor, k: int = 10, batch_size: int = 2048) -> Dict[str, object]:
        """The ``k`` nearest rows of every query ``vectors [Q, dim]``: ``{"indices": int64 [Q, k], "scores":
        fp32 [Q, k], "ids": Q lists of k names}``, CPU tensors in input order, best first.  Queries go through in
        batches of ``batch_size`` with no host synchronisation per batch: one at the end."""
        if not 1 <= k <= len(self):
            raise ValueError(f"k={k}: the index holds {len(self)} rows")
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        q = self._rows(vectors, "search")
        x = self.matrix
        nq = q.shape[0]
        cuda = self.device.type == "cuda"
        val = torch.empty((nq, k), dtype=torch.float32, pin_memory=cuda)
        idx = torch.empty((nq, k), dtype=torch.int32, pin_memory=cuda)
        fused = self._fused(k)
        for s in range(0, nq, batch_size):
            e = min(nq, s + batch_size)
            v, i = _ops.search_topk(q[s:e], x, k) if fused else _ops.search_topk_torch(q[s:e], x, k)
            val[s:e].copy_(v, non_blocking=True)
            idx[s:e].copy_(i, non_blocking=True)
        if cuda:
            torch.cuda.synchronize(self.device)
        idx = idx.long()
        return {"indices": idx, "scores": val, "ids": [[self.ids[j] for j in row] for row in idx.tolist()]}

    def scores(self, vectors: torch.Tensor) -> torch.Tensor:
        """The full score matrix ``[Q, N]`` fp32 on the CPU (all-against-all for small sets); at most 2^31
        elements.  On the fused path these are the bits the search selects on."""
        q = self._rows(vectors, "scores")
        nq, n = q.shape[0], len(self)
        if n < 1:
            raise ValueError("scores: the index is empty")
        if nq * n > MAX_SCORE_ELEMENTS:
            raise ValueError(f"scores: {nq} x {n} is more than 2^31 elements: use search()")
        if nq == 0:
            return torch.empty((0, n), dtype=torch.float32)
        x = self.matrix
        if self._fused(1):
            out = torch.empty((nq, n), dtype=torch.float32, device=self.device)
            _ops.search_topk(q, x, 1, scores=out)
            return out.cpu()
        return (q.float() @ x.float().t()).cpu()

    # ------------------------------------------------------------------------
    @classmethod
    def from_sequences(cls, pred, sequences: Sequence[str], ids: Optional[Sequence[str]] = None,
                       embedding: str = "global", metric: str = "cosine", truncate: bool = False,
                       device=None) -> "EmbeddingIndex":
        """An index of ``pred``'s (:class:`~.inference.Predictor`) ``embedding`` of ``sequences``, on ``device``
        (default: the predictor's)."""
        if embedding not in EMBEDDINGS:
            raise ValueError(f"embedding {embedding!r}: expected one of {EMBEDDINGS}")
        vec = pred.predict(list(sequences), outputs=(embedding,), truncate=truncate)[embedding]
        index = cls(vec.shape[1], metric=metric, embedding=embedding, device=device or pred.device)
        index.add(vec, ids)
        return index

    def search_sequences(self, pred, sequences: Sequence[str], k: int = 10, truncate: bool = False,
                         batch_size: int = 2048) -> Dict[str, object]:
        """:meth:`search` with the queries embedded by ``pred`` the way the rows were."""
        if self.embedding is None:
            raise ValueError("search_sequences: this index does not record which embedding its rows are")
        vec = pred.predict(list(sequences), outputs=(self.embedding,), truncate=truncate)[self.embedding]
        if vec.shape[1] != self.dim:
            raise ValueError(f"the model's {self.embedding!r} embedding has {vec.shape[1]} dimensions, the index "
                             f"{self.dim}")
        return self.search(vec, k=k, batch_size=batch_size)

    # ------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """Write the index as ``.npz`` (module docstring)."""
        rows = self.matrix.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
        meta = {"metric": self.metric, "embedding": self.embedding, "dim": self.dim, "version": FORMAT_VERSION}
        with open(path, "wb") as fh:                # a file object: np.savez would append ".npz" to a bare name
            np.savez(fh, rows=rows, ids=np.array(self.ids, dtype=np.str_), meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path: str, device="cpu", model=None) -> "EmbeddingIndex":
        """Read a file of :meth:`save`.  ``model``: the encoder the index will be used with; its embedding
        width is checked against the file's ``dim``."""
        with np.load(path, allow_pickle=False) as z:
            if not {"rows", "ids", "meta"} <= set(z.files):
                raise ValueError(f"{path}: not an embedding index (rows, ids, meta expected)")
            meta = json.loads(str(z["meta"]))
            rows, ids = z["rows"], [str(i) for i in z["ids"]]
        if meta.get("version") != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {meta.get('version')!r}, this code reads {FORMAT_VERSION}")
        if rows.dtype != np.uint16 or rows.ndim != 2 or rows.shape != (len(ids), meta["dim"]):
            raise ValueError(f"{path}: rows {rows.dtype} {rows.shape} do not match {len(ids)} ids of dim {meta['dim']}")
        index = cls(meta["dim"], metric=meta["metric"], embedding=meta["embedding"], device=device)
        if model is not None:
            index.check_model(model)
        if len(ids):
            bits = torch.from_numpy(rows.view(np.int16).copy()).view(torch.bfloat16)
            index._chunks = [bits.to(index.device)]       # already normalised and rounded: taken as stored
            index.ids = ids
        return index

    def check_model(self, model) -> None:
        """Raise ``ValueError`` when ``model``'s embedding of this index's kind has another width."""
        if self.embedding is None:
            return
        want = model.config["global_dim"] if self.embedding == "global" else model.config["local_dim"]
        if want != self.dim:
            raise ValueError(f"the index holds {self.embedding!r} embeddings of {self.dim} dimensions, the model's "
                             f"have {want}")
