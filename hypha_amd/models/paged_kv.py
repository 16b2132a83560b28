"""Paged KV cache for autoregressive serving.

The cache of a batch is a pool of fixed-size pages instead of one dense
[B, T_max, Hkv, D] slab (kv_cache.py): a sequence is charged the pages its
own length needs, not the batch's longest. A page is PAGE = 64 rows — the kv
tile of the decode and prefill kernels, so one staged tile is one page and
the kernels look a page id up once per tile (ops.attn_decode_paged,
ops.attn_prefill_paged, ops.kv_append_paged).

PageTable   one per batch, shared by every layer: the device block table
            int32 [B, max_pages] (logical row j of sequence b is row j % 64 of
            page table[b, j // 64]), its host mirror and the free list.
PagedKVCache one per layer: the pools k, v [n_pages, 64, Hkv, D] (bf16, or
            e4m3 with k_scale, v_scale [n_pages, 64, Hkv] fp32) — the bshd
            layout of KVCache with B := n_pages and T_alloc := 64.

Pages are reserved on the host before a call's first step (PageTable.reserve);
nothing is allocated while decoding, so a decode step stays graph-capturable
and a captured graph stays valid across calls: reserve rewrites the table in
place.
"""

from __future__ import annotations

import torch

from hypha_amd import ops
from hypha_amd.ops.reference import PAGE, gather_pages


class PagePoolExhausted(RuntimeError):
    """A reservation needs more pages than the pool holds."""


def pages_for(rows: int) -> int:
    return (int(rows) + PAGE - 1) // PAGE


class PageTable:
    def __init__(self, batch: int, max_pages: int, n_pages: int, device,
                 free_order=None):
        if batch < 1 or max_pages < 1 or n_pages < 1:
            raise ValueError("PageTable: batch, max_pages and n_pages must be >= 1")
        order = list(range(n_pages)) if free_order is None else [int(p) for p in free_order]
        if sorted(order) != list(range(n_pages)):
            raise ValueError("PageTable: free_order must be a permutation of "
                             "range(n_pages)")
        self.batch = batch
        self.max_pages = max_pages
        self.n_pages = n_pages
        self.device = torch.device(device)
        self._order = order
        self._free = list(order)  # handed out from the front
        self.host = torch.full((batch, max_pages), -1, dtype=torch.int32)
        self.table = self.host.to(self.device).clone()
        self._pos = (None, None)  # last (int, device tensor) of pos_tensor

    @property
    def max_rows(self) -> int:
        """Logical rows a sequence can address: also the parking position."""
        return self.max_pages * PAGE

    @property
    def pages_in_use(self) -> int:
        return self.n_pages - len(self._free)

    def reserve(self, rows) -> None:
        """rows: one row count per sequence. Frees every page held, then gives
        sequence b its first ceil(rows[b] / 64) pages in free_order; the other
        slots become -1. The device table is rewritten in place. Raises
        PagePoolExhausted, and changes nothing, when the pool is too small."""
        need = [pages_for(r) for r in torch.as_tensor(rows).reshape(-1).tolist()]
        if len(need) != self.batch:
            raise ValueError(f"reserve: {len(need)} row counts for a batch of "
                             f"{self.batch}")
        if min(need) < 0 or max(need) > self.max_pages:
            raise ValueError(f"reserve: a sequence needs {max(need)} pages, the "
                             f"table has {self.max_pages} slots")
        if sum(need) > self.n_pages:
            raise PagePoolExhausted(
                f"{sum(need)} pages needed for rows {list(rows)}, the pool "
                f"holds {self.n_pages}")
        free = list(self._order)
        host = torch.full_like(self.host, -1)
        for b, n in enumerate(need):
            host[b, :n] = torch.tensor(free[:n], dtype=torch.int32)
            free = free[n:]
        self._free = free
        self.host = host
        self.table.copy_(host)

    def pos_tensor(self, pos: int) -> torch.Tensor:
        """int64 [1] on the device holding pos; the last one is kept, so the
        layers of one chunk share a single upload."""
        if self._pos[0] != pos:
            self._pos = (pos, torch.tensor([pos], dtype=torch.long, device=self.device))
        return self._pos[1]


class PagedKVCache:
    __slots__ = ("table", "k", "v", "quant", "k_scale", "v_scale")

    def __init__(self, table: PageTable, n_kv_heads: int, head_dim: int, device,
                 dtype=torch.bfloat16, quant: str | None = None):
        self.table = table
        self.quant = quant
        shape = (table.n_pages, PAGE, n_kv_heads, head_dim)
        if quant == "fp8":
            self.k = torch.zeros(shape, device=device, dtype=torch.float8_e4m3fn)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.ones(shape[:3], device=device, dtype=torch.float32)
            self.v_scale = torch.ones_like(self.k_scale)
        elif quant is None:
            self.k = torch.zeros(shape, device=device, dtype=dtype)
            self.v = torch.zeros_like(self.k)
            self.k_scale = self.v_scale = None
        else:
            raise ValueError(f"unknown KV quant mode {quant!r}")

    def append_chunk(self, k: torch.Tensor, v: torch.Tensor, pos: int,
                     seq_lens=None) -> None:
        """Prefill chunk: k/v [B, s, Hkv, D], row i at position pos + i (host
        int). With seq_lens (int32 [B]) the rows at or past a sequence's
        length are not written: a short sequence owns no page for them."""
        ops.kv_append_paged(k, v, self.k, self.v, self.table.table,
                            self.table.pos_tensor(pos), self.k_scale, self.v_scale,
                            lens=seq_lens)

    def append_rows(self, k: torch.Tensor, v: torch.Tensor, pos: torch.Tensor) -> None:
        """Decode step, the contract of KVCache.append_rows: k/v [B, 1, Hkv, D]
        go to logical row pos[b] of sequence b (int64 [B] on the device). A
        pos[b] outside [0, max_pages * 64) writes nothing (the parking position
        of a finished sequence). Graph-capturable on the native path."""
        if k.shape[1] != 1 or pos.shape != (k.shape[0],):
            raise ValueError("append_rows: k/v must be [B, 1, Hkv, D] and pos [B]")
        ops.kv_append_paged(k, v, self.k, self.v, self.table.table, pos,
                            self.k_scale, self.v_scale)

    def gather(self, n_rows: int | None = None):
        """Contiguous copies (k, v, k_scale, v_scale) [B, n_rows, ...] of the
        batch's logical caches (scales None for a bf16 pool)."""
        t = self.table.table
        ks = vs = None
        if self.quant == "fp8":
            ks = gather_pages(self.k_scale, t, n_rows)
            vs = gather_pages(self.v_scale, t, n_rows)
        return gather_pages(self.k, t, n_rows), gather_pages(self.v, t, n_rows), ks, vs


def kv_bytes(rows: int, n_layers: int, n_kv_heads: int, head_dim: int,
             quant: str | None, elem_bytes: int = 2) -> int:
    """Bytes of K and V (and fp8 row scales) for that many cache ROWS over all
    layers: a count from shapes, for either layout."""
    per_row = n_kv_heads * (head_dim * (1 if quant == "fp8" else elem_bytes)
                            + (4 if quant == "fp8" else 0))
    return 2 * n_layers * rows * per_row
