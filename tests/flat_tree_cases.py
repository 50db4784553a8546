"""TEST INFRASTRUCTURE (a helper, not a test module): the tree all-reduce stated as include/nexr.h states it for
nexrFlatTreeAllReduce: a tree compiled into a program of LEAF / JOIN / PUSH / MERGE, an interpreter of that
program over numpy with a step callback, and the count of values the program keeps alive (tests/test_flat_tree.py
on the CPU, tests/test_flat_tree_gpu.py on the MI355X).

numpy only; it never imports the library under test or the oracle. The caller hands in the trees (links as
oracle.ring.tree_topology gives them: (up, [down...]) per rank), the channel parts and the step function.

A step function is
    step(x, vals, post) -> v
one reduce-copy step with the rank's own input x (an array of the element's unsigned integer, or None where the
step has none: a MERGE) and the values `vals` that earlier steps returned, in the order [saved accumulator,
child's value] for a MERGE and [first child's value] for a JOIN; which of them is the first operand is the
protocol's, so the step function's, business, as is what travels between two steps (the LL oracles hand their wire
lines on). post is True for the program's last instruction (the root's last step), whose return value is the
result's elements."""
from __future__ import annotations

from typing import Callable, List, Sequence

import numpy as np

LEAF, JOIN, PUSH, MERGE = range(4)
SLOTS = 8  # NEXR_FLAT_TREE_SLOTS


def compile_tree(links: Sequence[tuple]) -> list:
    """[(opcode, rank)] for `links`: from the root, down[0]'s value first, then the rank's own input (JOIN), then
    for every further child PUSH, the child, MERGE. A rank without children is a LEAF."""
    roots = [r for r, (up, _d) in enumerate(links) if up == -1]
    assert len(roots) == 1, roots
    code = []

    def emit(r):
        down = list(links[r][1])
        if not down:
            code.append((LEAF, r))
            return
        emit(down[0])
        code.append((JOIN, r))
        for k in down[1:]:
            code.append((PUSH, 0))
            emit(k)
            code.append((MERGE, 0))

    emit(roots[0])
    assert sorted(r for op, r in code if op in (LEAF, JOIN)) == list(range(len(links)))
    assert len(code) <= max(1, 3 * len(links) - 2)
    return code


def encode(code: Sequence[tuple]) -> bytes:
    """One byte an instruction: opcode << 6 | rank."""
    return bytes(op << 6 | r for op, r in code)


def live_values(code: Sequence[tuple]) -> int:
    """The most values alive at once: the accumulator and the saved ones."""
    depth, most = 0, 1
    for op, _r in code:
        if op == PUSH:
            depth += 1
            most = max(most, depth + 1)
        elif op == MERGE:
            depth -= 1
    assert depth == 0
    return most


def interpret(code: Sequence[tuple], inputs: List[np.ndarray], step: Callable) -> np.ndarray:
    """The program over whole arrays: what the last instruction's step returns."""
    acc, stack = None, []
    last = len(code) - 1
    for i, (op, r) in enumerate(code):
        if op == LEAF:
            acc = step(np.ascontiguousarray(inputs[r]), [], i == last)
        elif op == JOIN:
            acc = step(np.ascontiguousarray(inputs[r]), [acc], i == last)
        elif op == PUSH:
            stack.append(acc)
        else:
            acc = step(None, [stack.pop(), acc], i == last)
    assert not stack
    return acc


def model(inputs: List[np.ndarray], parts: Sequence[tuple], trees: Sequence[Sequence[tuple]], step: Callable) -> list:
    """Every rank's expected output: `parts` are (offset, count, tree) in elements and tile the buffer; each part
    runs the program of its tree."""
    n = len(inputs)
    out = np.empty_like(inputs[0])
    codes = [compile_tree(t) for t in trees]
    at = 0
    for offset, cnt, t in parts:
        assert offset == at and cnt > 0, (parts, at)
        sl = slice(offset, offset + cnt)
        out[sl] = np.asarray(interpret(codes[t], [x[sl] for x in inputs], step)).view(out.dtype).reshape(-1)
        at += cnt
    assert at == out.size
    return [out] * n
