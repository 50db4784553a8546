"""TEST INFRASTRUCTURE (a helper, not a test module): where the arena of one tests/ring_modes_cases.py call lives
in host memory and what of it is registered, for tests/test_ring_host_memory.py (CPU) and
tests/test_ring_host_memory_gpu.py (MI355X). numpy only; it never imports the library under test: the caller hands
in `register(address, bytes) -> handle` and `deregister(handle)`.

One page-aligned anonymous mapping serves a whole test (mapping_bytes: the largest arena of its plan plus two
pages); every call's arena0 is copied into it at the offset place() computes, which keeps the arena start a
multiple of 16 (rm aligns every user buffer to 16 bytes from the arena start). The kinds, PAGE = mmap.PAGESIZE:

  pageable    the arena at PAGE + 48 of the mapping; nothing registered.
  registered  the same offset; the whole mapping registered: every user pointer is an interior, non-page-aligned
              pointer of one cache entry.
  pinned      the arena at PAGE + 48 of memory that the HIP runtime pinned and the library never saw (the caller's,
              e.g. a torch pin_memory() byte tensor of mapping_bytes); nothing registered.
  split       the arena placed so that a cut inside it falls on a page boundary of the mapping, and only [mapping
              base, that boundary) registered. The cut is a multiple of 16 from the arena start (the page boundary
              and the arena start both are) inside the user buffer at the arena's middle (split_cut), so the
              registration ends inside some rank's user buffer: the buffers below it are read in place, the one
              it divides is read in place up to the last slice that ends below it, and the rest is staged.

The arena's own middle, (arena bytes // 2) & ~15, would not do as the cut: rm lays the ranks' buffers out one after
the other, all of one size, so for every even number of ranks, and at 3 ranks out of place, the middle of the arena
is in the guard between two buffers, and no buffer would be divided."""
from __future__ import annotations

import mmap
from contextlib import contextmanager
from typing import Callable, NamedTuple, Optional

import numpy as np

import ring_modes_cases as rm

PAGE = mmap.PAGESIZE
KINDS = ("pageable", "registered", "pinned", "split")
OFFSET = PAGE + 48   # of every kind but split


def page_ceil(v: int) -> int:
    return (v + PAGE - 1) // PAGE * PAGE


def mapping_bytes(largest_arena: int) -> int:
    return page_ceil(largest_arena) + 2 * PAGE


class Placement(NamedTuple):
    kind: str
    offset: int                # of the arena's first byte in its memory
    registered: Optional[int]  # bytes registered from the mapping's base (None: nothing)
    cut: Optional[int]         # split: the arena offset at which the registration ends


def split_cut(arena_bytes: int, regions) -> int:
    """The arena offset at which split's registration ends. Of call.regions' buffers that start at a multiple of
    16, the one that holds the arena's middle byte, else the nearest to it (the larger of two equally near, then
    the lower); the cut is its own middle rounded down to 16 bytes, and 16 bytes into it where that would be its
    first byte. A buffer of 16 bytes or fewer cannot hold a cut that is a multiple of 16: there the cut is its
    first byte, and the buffer lies wholly above it."""
    mid = arena_bytes // 2

    def key(reg):
        _rank, _kind, off, nbytes = reg
        dist = 0 if off <= mid < off + nbytes else min(abs(mid - off), abs(mid - (off + nbytes - 1)))
        return (dist, -nbytes, off)
    _rank, _kind, off, nbytes = min((r for r in regions if r[2] % 16 == 0), key=key)
    return off + (max(16, (nbytes // 2) & ~15) if nbytes > 16 else 0)


def place(kind: str, arena_bytes: int, mapping_size: int, regions=None) -> Placement:
    if kind == "split":
        mid = split_cut(arena_bytes, regions)
        boundary = page_ceil(mid) + PAGE    # the first page boundary that leaves a whole page before the arena
        pl = Placement(kind, boundary - mid, boundary, mid)
    else:
        pl = Placement(kind, OFFSET, mapping_size if kind == "registered" else None, None)
    assert kind in KINDS and pl.offset % 16 == 0 and pl.offset >= PAGE, pl
    assert pl.offset + arena_bytes <= mapping_size, (pl, arena_bytes, mapping_size)
    return pl


def cut_region(call, pl: Placement):
    """The (rank, kind, offset, bytes) of call.regions that split's cut lies strictly inside, or None (the cut
    is in a guard or on a buffer's first byte)."""
    for reg in call.regions:
        if reg[2] < pl.cut < reg[2] + reg[3]:
            return reg
    return None


class Mapping:
    """One anonymous mapping, page-aligned. `pinned` is the caller's runtime-pinned memory of at least the same
    size as a uint8 array (None where the test has no such kind)."""

    def __init__(self, nbytes: int, pinned: Optional[np.ndarray] = None):
        assert nbytes % PAGE == 0
        self.m = mmap.mmap(-1, nbytes)
        self.buf = np.frombuffer(self.m, dtype=np.uint8)
        self.base = self.buf.ctypes.data
        assert self.base % PAGE == 0
        self.size = nbytes
        self.pinned = pinned
        assert pinned is None or (pinned.dtype == np.uint8 and pinned.size >= nbytes)

    def memory(self, pl: Placement) -> np.ndarray:
        return self.pinned if pl.kind == "pinned" else self.buf

    @contextmanager
    def placed(self, kind: str, call, register: Optional[Callable] = None, deregister: Optional[Callable] = None,
               content: Optional[np.ndarray] = None):
        """The call's arena0 (or `content`, of the same size) copied to its place, with what the kind registers
        registered for the duration: yields (placement, the arena's address, a view of the arena in place)."""
        arena0 = call.arena0 if content is None else content
        assert arena0.size == call.arena0.size
        pl = place(kind, arena0.size, self.size, call.regions)
        mem = self.memory(pl)
        view = mem[pl.offset:pl.offset + arena0.size]
        view[:] = arena0
        handle = register(self.base, pl.registered) if pl.registered else None
        try:
            yield pl, mem.ctypes.data + pl.offset, view
        finally:
            if handle is not None:
                deregister(handle)


def largest_arena(calls) -> int:
    return max(c.arena0.size for c in calls)


# ---- what both test modules ask of a call --------------------------------------------------------------------------
ONE_RANK_COUNTS = (("1", lambda p: 1), ("p-1", lambda p: p - 1), ("p+1", lambda p: p + 1), ("4099", lambda p: 4099))


def one_rank_plan() -> list:
    """The calls on a communicator of one rank: all six collectives at 1, p - 1, p + 1 and 4,099 elements, out of
    place and in place, over rm.PAIRS (p - 1 = 1 of the 8-byte types is not repeated). k mod 11 is the pair's
    index, as in rm.spec."""
    out = []
    for coll in rm.COLLECTIVES:
        for j, (dt, op) in enumerate(rm.PAIRS):
            seen = set()
            for edge, f in ONE_RANK_COUNTS:
                count = f(16 // rm.esz_of(dt))
                if count in seen:
                    continue
                seen.add(count)
                for in_place in (False, True):
                    out.append(rm.Spec(len(out) * len(rm.PAIRS) + j, coll, edge, count, dt, op, in_place, 0))
    return out


def direct_expectation(sp):
    """With set_direct: direct slices after all-gather, broadcast and out-of-place all-reduce (True), none after
    reduce-scatter, reduce and in-place all-reduce (False); the tree does not report (None)."""
    if sp.collective == "tree":
        return None
    return sp.collective in ("all_gather", "broadcast") or (sp.collective == "all_reduce" and not sp.in_place)


def check_direct(comm, sp, context) -> None:
    """comm.direct_slices() after the call `sp` under set_direct(True) against direct_expectation."""
    want = direct_expectation(sp)
    if want is None:
        return
    d, f = comm.direct_slices()
    assert (d > 0) == want, (context, sp.what(), d, f)
