"""Exact top-k neighbours by inner product (``csrc/search.hip``).

``score[q, r] = sum_d float(Q[q, d]) * float(X[r, d])`` over bf16 operands, accumulated in fp32; the result of a
search is, per query, the first ``k`` database rows of the total order (score descending, then index ascending).

* :func:`search_topk` -- the fused path: one launch of ``pbx_search_topk`` forms 32 x 32 score tiles on the bf16
  MFMA and keeps every query's best ``k`` as the database streams by, per split of the database; the ``S`` lists of
  a query are then merged by :func:`.infer_heads.row_topk` (ties by ascending position in the concatenated lists,
  which is ascending database index) and one ``gather``.  The ``[nq, n]`` score matrix is never stored, unless the
  caller passes ``scores`` to receive it (the very bits the selection used).
* :func:`search_topk_torch` -- the definition on any device, in chunks of database rows.

A score's bits depend on the two rows alone (not on the split count, the number of queries or the place in a
tile), so results are repeatable and the stored matrix is the same for every launch shape.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .infer_heads import TOPK_MAX_COLS, TOPK_MAX_K, row_topk

F32 = torch.float32
MAX_K = TOPK_MAX_K              # a list is ranked one member per lane of a wave
MAX_D = 1024                    # the query fragments of a wave stay in registers: D / 16 fragments of 4 VGPRs
MAX_N = 2 ** 31 - 1             # indices are int32
QUERY_TILE = 128                # queries per workgroup (4 waves of 32)
ROW_TILE = 32                   # database rows per tile; a split is a run of whole tiles


def search_supported(D: int, k: int, n: int) -> bool:
    """Whether :func:`search_topk` takes ``k`` neighbours among ``n`` rows of ``D`` columns."""
    return 16 <= D <= MAX_D and D % 16 == 0 and 1 <= n <= MAX_N and 1 <= k <= min(MAX_K, n)


def default_splits(nq: int, n: int, k: int, device=None) -> int:
    """Splits of the database for ``nq`` queries: enough workgroups to fill the chip (two per CU when a single
    query tile streams the database, which is then bandwidth-bound; one per CU otherwise, because every split
    pays for filling its own lists), within ``S * k <= 16384`` and one tile per split at least."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    nqt = (nq + QUERY_TILE - 1) // QUERY_TILE
    want = (2 * cus if nqt == 1 else cus + nqt - 1) // nqt
    tiles = (n + ROW_TILE - 1) // ROW_TILE
    return max(1, min(want, TOPK_MAX_COLS // k, tiles))


def _operand(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2 or t.dtype != torch.bfloat16:
        raise ValueError(f"search_topk: {name} must be a 2-D bf16 matrix")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 8 != 0 or t.data_ptr() % 16 != 0:
        t = t.clone(memory_format=torch.contiguous_format)       # rows must be 16-byte aligned
    return t


def search_topk(q_bf: torch.Tensor, x_bf: torch.Tensor, k: int, splits: Optional[int] = None,
                scores: Optional[torch.Tensor] = None, order: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(values [nq, k] fp32, indices [nq, k] int32)`` of the ``k`` best rows of ``x_bf [n, D]`` for every row
    of ``q_bf [nq, D]`` (bf16, CUDA, unit column stride; any 16-byte aligned row stride): score descending, equal
    scores by ascending index.  ``splits``: parts of the database searched by separate workgroups (default:
    :func:`default_splits`); the result does not depend on it.  ``scores``: an fp32 ``[nq, n]`` tensor or view with
    unit column stride that receives every score.  ``order``: which index varies fastest over the grid, 0 the query
    tile, 1 the split (the default: 0.4 to 2.4 % faster with 16 query tiles, tools/search_bench.py); the result does
    not depend on it.
    Raises ``ValueError`` outside :func:`search_supported`, before any launch.  Scores must be finite."""
    q, x = _operand(q_bf, "q_bf"), _operand(x_bf, "x_bf")
    nq, D = q.shape
    n = x.shape[0]
    if x.shape[1] != D:
        raise ValueError(f"search_topk: queries have {D} columns, the database {x.shape[1]}")
    if not search_supported(D, k, n):
        raise ValueError(f"search_topk: D={D}, k={k}, n={n} is outside the kernel's range (D a multiple of 16 in "
                         f"16 .. {MAX_D}, 1 <= k <= min({MAX_K}, n), n <= {MAX_N})")
    if nq < 1:
        raise ValueError("search_topk: no queries")
    if not q.is_cuda or q.device != x.device:
        raise ValueError("search_topk: the operands must be on one CUDA device (search_topk_torch is the "
                         "definition on any device)")
    S = default_splits(nq, n, k, q.device) if splits is None else int(splits)
    if S < 1 or S * k > TOPK_MAX_COLS:
        raise ValueError(f"search_topk: splits={S} with k={k}: expected 1 <= splits and splits * k <= {TOPK_MAX_COLS}")
    if order not in (0, 1):
        raise ValueError("search_topk: order is 0 or 1")
    if scores is not None:
        if (scores.shape != (nq, n) or scores.dtype != F32 or scores.device != q.device or scores.stride(1) != 1
                or scores.stride(0) < n):
            raise ValueError(f"search_topk: scores must be fp32 [{nq}, {n}] with unit column stride on {q.device}")
    pval = torch.empty((nq, S, k), dtype=F32, device=q.device)
    pidx = torch.empty((nq, S, k), dtype=torch.int32, device=q.device)
    _lib.call("pbx_search_topk", q.data_ptr(), q.stride(0), x.data_ptr(), x.stride(0), nq, n, D, int(k), S,
              pval.data_ptr(), pidx.data_ptr(), _lib.ptr(scores), 0 if scores is None else scores.stride(0),
              int(order), _lib.stream_ptr(q.device))
    if S == 1:
        return pval.view(nq, k), pidx.view(nq, k)
    # exact merge: inside a list equal scores stand in ascending index and every index of split j is below
    # every index of split j + 1, so "ties by ascending position" here is "ties by ascending database index"
    val, pos = row_topk(pval.view(nq, S * k), k)
    return val, pidx.view(nq, S * k).gather(1, pos.long())


def search_topk_torch(q_bf: torch.Tensor, x_bf: torch.Tensor, k: int,
                      chunk: int = 65536) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`search_topk` by definition, on any device and for any ``D`` and ``k <= n``: per chunk of ``chunk``
    database rows ``q.float() @ x.float().T``, and a running stable top-k in the same total order.  Never holds
    more than ``[nq, chunk + k]`` scores."""
    if q_bf.dim() != 2 or x_bf.dim() != 2 or q_bf.shape[1] != x_bf.shape[1]:
        raise ValueError("search_topk_torch: expected [nq, D] queries and an [n, D] database")
    nq, n = q_bf.shape[0], x_bf.shape[0]
    if not 1 <= k <= n:
        raise ValueError(f"search_topk_torch: k={k} of n={n} rows")
    if chunk < 1:
        raise ValueError("search_topk_torch: chunk must be positive")
    qf = q_bf.float()
    dev = q_bf.device
    run_v = torch.empty((nq, 0), dtype=F32, device=dev)
    run_i = torch.empty((nq, 0), dtype=torch.int64, device=dev)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        s = qf @ x_bf[c0:c1].float().t()
        # the kept candidates (lower indices, already in order) stand before the chunk (ascending index): a
        # stable descending sort breaks every tie by ascending index
        cand_v = torch.cat([run_v, s], dim=1)
        cand_i = torch.cat([run_i, torch.arange(c0, c1, device=dev).expand(nq, -1)], dim=1)
        sv, order = torch.sort(cand_v, dim=1, descending=True, stable=True)
        run_v = sv[:, :k].contiguous()
        run_i = cand_i.gather(1, order[:, :k])
    return run_v, run_i.to(torch.int32)
