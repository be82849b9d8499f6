"""Item iterators of a SIMD template.

The reference hands ExaModels a ``Vector{NamedTuple}`` per template
(``/root/reference/src/transform.jl:31, 440-451, 538-544, 584-591, 632, 670``): one
record per item with integer support indices (``group_idxK``, ``i1``/``i2``),
Float64 support values (``ip…``/``dp…``), quadrature coefficients ``c`` and stencil
coefficients ``d_argK``.  At 10⁶ supports an array-of-records is exactly the
re-read traffic the device path must avoid, so :class:`Items` keeps the same
information *structurally*:

* an item box ``dims`` (first coordinate fastest — the order
  ``Iterators.product`` yields at ``transform.jl:445``),
* integer fields that are affine in the item coordinates (``group_idx = 1 + k``)
  or gathered from an explicit int64 column,
* float fields gathered from a (shared, de-duplicated) float64 array.

``records()`` re-materialises the reference's list-of-NamedTuples for small cases
(tests compare against it).

The blob's item box has at most three axes (``include/iem_blob.h``).  A product of more
groups (``Iterators.product(itrs...)`` over four or more) is kept here with one logical
axis per factor and *folded* when a template is compiled (:func:`fold_runs`,
:meth:`Items.fold`): adjacent axes merge into runs, each run one box axis of extent
∏ nᵢ in mixed-radix order (first factor fastest), so item order is unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_DIMS = 3          # axes of the blob's item box

# virtual grid ids of folded runs (box axes that merge several groups): a range no other grid hint
# uses (groups < 1000, collocation 1000+g / 2000+g / 3000+g)
RUN_GRID_LO, RUN_GRID_HI = 3500, 4094


def run_grid_id(groups: Sequence[int]) -> int:
    """Grid hint of a merged run over (the grids) ``groups``: deterministic, so templates folded the
    same way share it (a scheduling hint only — a collision costs nothing but fusion)."""
    h = 0
    for g in groups:
        h = (h * 131 + int(g) + 1) % 1000003
    return RUN_GRID_LO + h % (RUN_GRID_HI - RUN_GRID_LO)


def fold_runs(dims: Sequence[int], free: Sequence[bool]) -> List[Tuple[int, int]]:
    """Partition ``len(dims)`` logical axes into at most three runs of adjacent axes ``[lo, hi)``.

    An axis that is not ``free`` (restricted by a template: a derivative's pref axis, a
    ``select``/``take``, a collocation box) must be alone in its run or its slowest digit, so that
    its item set stays a contiguous interval of the run coordinate.  The first valid partition in
    the order (fast axes alone, slow axes merged) wins; with one restricted axis one always exists."""
    n = len(dims)
    if n <= MAX_DIMS:
        return [(d, d + 1) for d in range(n)]
    for c1 in range(1, n - 1):
        for c2 in range(c1 + 1, n):
            runs = [(0, c1), (c1, c2), (c2, n)]
            if all(free[d] or hi - lo == 1 or d == hi - 1 for lo, hi in runs for d in range(lo, hi)):
                return runs
    raise ValueError(f"cannot fold a product of {n} item axes into {MAX_DIMS} runs: the restricted axes "
                     f"{[d for d in range(n) if not free[d]]} do not each end a run")


class Fold:
    """Map of logical axes onto the runs of :func:`fold_runs`: axis ``d`` is digit
    ``(K_r // stride[d]) % dims[d]`` of run coordinate ``K_r``, ``r = run_of[d]``."""

    def __init__(self, dims: Sequence[int], runs: Sequence[Tuple[int, int]]):
        self.dims = tuple(int(n) for n in dims)
        self.runs = [tuple(r) for r in runs]
        self.run_of, self.stride, self.ext = [], [], []
        for r, (lo, hi) in enumerate(self.runs):
            s = 1
            for d in range(lo, hi):
                self.run_of.append(r)
                self.stride.append(s)
                s *= self.dims[d]
            self.ext.append(s)

    def digit(self, d: int) -> np.ndarray:
        """Logical coordinate ``k_d`` at every run coordinate of its run (length ``ext[run]``)."""
        r = self.run_of[d]
        return (np.arange(self.ext[r], dtype=np.int64) // self.stride[d]) % self.dims[d]

    def collapse(self, steps: Sequence[int]) -> Optional[Tuple[int, ...]]:
        """Per-run steps when ``Σ steps[d]·k_d`` is affine in the run coordinates (the steps of every
        run are proportional to its mixed-radix strides), else None."""
        out = []
        for r, (lo, hi) in enumerate(self.runs):
            live = [d for d in range(lo, hi) if self.dims[d] > 1]
            c = int(steps[live[0]]) // self.stride[live[0]] if live else 0
            if any(int(steps[d]) != c * self.stride[d] for d in range(lo, hi) if self.dims[d] > 1):
                return None
            out.append(c)
        return tuple(out)

    def touched(self, steps: Sequence[int]) -> List[int]:
        return sorted({self.run_of[d] for d in range(len(self.dims)) if steps[d] != 0 and self.dims[d] > 1})

    def over_runs(self, runs: Sequence[int], fn) -> Tuple[np.ndarray, Tuple[int, ...]]:
        """``fn(k)`` (k: logical coordinates, broadcast arrays) tabulated over the box of ``runs``
        (first run fastest) and the steps that read that table back."""
        shape = [self.ext[r] for r in reversed(runs)]
        k = [np.zeros((), dtype=np.int64)] * len(self.dims)
        for j, r in enumerate(runs):
            lo, hi = self.runs[r]
            for d in range(lo, hi):
                sh = [1] * len(runs)
                sh[len(runs) - 1 - j] = self.ext[r]
                k[d] = self.digit(d).reshape(sh)
        col = np.broadcast_to(fn(k), shape).reshape(-1)
        steps, s = [0] * len(self.runs), 1
        for r in runs:
            steps[r] = s
            s *= self.ext[r]
        return np.ascontiguousarray(col), tuple(steps)

    def field(self, f: "Field") -> "Field":
        """``f`` over the folded box: affine in the run coordinates when it can be, else a gather
        from a column over the runs it depends on (a short column when that is one run)."""
        c = self.collapse(f.steps)
        if c is not None:
            return Field(f.kind, f.mode, f.base, c, f.arr)
        def fn(k):
            idx = f.base + sum(int(f.steps[d]) * k[d] for d in range(len(self.dims)))
            return idx if f.mode == "affine" else f.arr[idx]
        col, steps = self.over_runs(self.touched(f.steps), fn)
        col = col.astype(np.int64 if f.kind == "int" else np.float64)
        return Field(f.kind, "gather", 0, steps, col)


@dataclass(frozen=True)
class Field:
    """value(k) = base + Σ step[d]·k_d            (mode 'affine', integer fields)
    value(k) = arr[base + Σ step[d]·k_d]          (mode 'gather')"""

    kind: str  # 'int' | 'float'
    mode: str  # 'affine' | 'gather'
    base: int
    steps: Tuple[int, ...]
    arr: Optional[np.ndarray] = None

    def values(self, dims: Tuple[int, ...]) -> np.ndarray:
        """All item values in item order (first coordinate fastest)."""
        idx = np.full((), self.base, dtype=np.int64)
        for d, n in enumerate(dims):
            shape = [1] * len(dims)
            shape[len(dims) - 1 - d] = n
            idx = idx + (self.steps[d] * np.arange(n, dtype=np.int64)).reshape(shape)
        idx = np.broadcast_to(idx, tuple(reversed(dims))).reshape(-1)
        return idx if self.mode == "affine" else self.arr[idx]

    def _pad(self, before: int, after: int) -> "Field":
        return Field(self.kind, self.mode, self.base, (0,) * before + self.steps + (0,) * after, self.arr)


class Items:
    """Structured item iterator (see module docstring)."""

    def __init__(self, dims: Sequence[int], fields: Dict[str, Field],
                 grid: Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]] = None,
                 free: Optional[Sequence[bool]] = None):
        self.dims = tuple(int(n) for n in dims)
        assert len(self.dims) >= 1   # more than MAX_DIMS: a product that fold() turns into a box
        self.fields = dict(fields)
        for f in self.fields.values():
            assert len(f.steps) == len(self.dims)
        # fusion hint: (group ids per dim, grid origin per dim); None = not on a support grid
        self.grid = grid
        # per axis: the whole base iterator of a group, in support order (may merge with the next axis)
        self.free = tuple(bool(v) for v in free) if free is not None else (False,) * len(self.dims)

    # ---- constructors --------------------------------------------------
    @staticmethod
    def single() -> "Items":
        """``[(;)]`` — the one-item iterator of a finite template (transform.jl:440)."""
        return Items((1,), {}, grid=((), ()))

    @staticmethod
    def from_supports(index_name: str, n: int, values: Dict[str, np.ndarray],
                      group_id: Optional[int] = None) -> "Items":
        """Base iterator of one infinite-parameter group (transform.jl:31):
        ``(group_idx = i, alias = support value…)`` for ``i = 1..n``."""
        fields = {index_name: Field("int", "affine", 1, (1,))}
        for name, arr in values.items():
            arr = np.ascontiguousarray(arr, dtype=np.float64)
            assert arr.shape == (n,)
            fields[name] = Field("float", "gather", 0, (1,), arr)
        grid = ((group_id,), (0,)) if group_id is not None else None
        return Items((n,), fields, grid=grid, free=(True,))

    @staticmethod
    def from_records(records: Sequence[dict]) -> "Items":
        """Explicit list of NamedTuple-like dicts (any iterator the structured
        constructors cannot express, e.g. after a domain-restriction filter).
        Integer columns that form an arithmetic progression become affine fields."""
        n = len(records)
        if n == 0:
            raise ValueError("empty item iterator")
        fields: Dict[str, Field] = {}
        for name in records[0].keys():
            col = [r[name] for r in records]
            if all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in col):
                a = np.asarray(col, dtype=np.int64)
                step = int(a[1] - a[0]) if n > 1 else 0
                if n == 1 or np.all(np.diff(a) == step):
                    fields[name] = Field("int", "affine", int(a[0]), (step,))
                else:
                    fields[name] = Field("int", "gather", 0, (1,), a)
            else:
                fields[name] = Field("float", "gather", 0, (1,), np.asarray(col, dtype=np.float64))
        return Items((n,), fields)

    # ---- combinators -----------------------------------------------------
    def __len__(self) -> int:
        return int(np.prod(self.dims))

    def product(self, other: "Items") -> "Items":
        """``vec([merge(i...) for i in Iterators.product(self, other)])`` — self's
        coordinate runs fastest; on a field-name clash ``other`` wins (``merge``)."""
        na, nb = len(self.dims), len(other.dims)
        dims = self.dims + other.dims
        fields = {k: f._pad(0, nb) for k, f in self.fields.items()}
        fields.update({k: f._pad(na, 0) for k, f in other.fields.items()})
        grid = None
        if self.grid is not None and other.grid is not None:
            grid = (self.grid[0] + other.grid[0], self.grid[1] + other.grid[1])
        return Items(dims, fields, grid, free=self.free + other.free)

    def fold(self, runs: Sequence[Tuple[int, int]]) -> "Items":
        """The same items over the box of :func:`fold_runs` ``runs`` (every field value, hence
        ``records()``, unchanged).  A merged run's grid hint is a virtual grid
        (:func:`run_grid_id`) whose origin is its slowest digit's."""
        F = Fold(self.dims, runs)
        fields = {k: F.field(f) for k, f in self.fields.items()}
        grid = None
        if self.grid is not None and len(self.grid[0]) == len(self.dims):
            gids, org = [], []
            for r, (lo, hi) in enumerate(F.runs):
                if hi - lo == 1:
                    gids.append(self.grid[0][lo])
                    org.append(self.grid[1][lo])
                else:
                    if any(self.grid[1][d] for d in range(lo, hi - 1)):
                        break   # (a restricted axis never sits inside a run; no hint then)
                    gids.append(run_grid_id(self.grid[0][lo:hi]))
                    org.append(self.grid[1][hi - 1] * F.stride[hi - 1])
            else:
                grid = (tuple(gids), tuple(org))
        return Items(tuple(F.ext), fields, grid)

    def select(self, start: int, count: int) -> "Items":
        """Contiguous 0-based sub-range of a 1-D iterator (``srt_itr[idxs]`` at
        transform.jl:538 when ``idxs`` is a range)."""
        assert len(self.dims) == 1 and 0 <= start and start + count <= self.dims[0]
        fields = {k: Field(f.kind, f.mode, f.base + f.steps[0] * start, f.steps, f.arr)
                  for k, f in self.fields.items()}
        grid = None
        if self.grid is not None and self.grid[0]:
            grid = (self.grid[0], (self.grid[1][0] + start,))
        return Items((count,), fields, grid)

    def take(self, idxs: Sequence[int]) -> "Items":
        """Arbitrary 0-based subset of a 1-D iterator (contiguous → :meth:`select`)."""
        idxs = np.asarray(idxs, dtype=np.int64)
        if len(idxs) and np.all(np.diff(idxs) == 1):
            return self.select(int(idxs[0]), len(idxs))
        assert len(self.dims) == 1
        fields = {}
        for k, f in self.fields.items():
            vals = f.values(self.dims)[idxs]
            if f.kind == "int":
                fields[k] = Field("int", "gather", 0, (1,), np.ascontiguousarray(vals, dtype=np.int64))
            else:
                fields[k] = Field("float", "gather", 0, (1,), np.ascontiguousarray(vals, dtype=np.float64))
        return Items((len(idxs),), fields)

    def filter(self, mask: np.ndarray) -> "Items":
        """Keep items where ``mask`` (item order) is true (transform.jl:448-451)."""
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        assert mask.shape[0] == len(self)
        flat = self.flatten()
        return flat.take(np.nonzero(mask)[0])

    def flatten(self) -> "Items":
        """Same items as a 1-D iterator with explicit columns where needed."""
        if len(self.dims) == 1:
            return self
        n = len(self)
        fields = {}
        for k, f in self.fields.items():
            vals = np.ascontiguousarray(f.values(self.dims))
            fields[k] = Field(f.kind, "gather", 0, (1,), vals.astype(np.int64 if f.kind == "int" else np.float64))
        return Items((n,), fields)

    def with_float(self, name: str, values: np.ndarray) -> "Items":
        """Add one Float64 per item of a 1-D iterator (``c``, ``d_argK``)."""
        assert len(self.dims) == 1
        arr = np.ascontiguousarray(values, dtype=np.float64)
        assert arr.shape == (self.dims[0],)
        fields = dict(self.fields)
        fields[name] = Field("float", "gather", 0, (1,), arr)
        return Items(self.dims, fields, self.grid, self.free)

    def with_int_affine(self, name: str, base: int, step: int) -> "Items":
        assert len(self.dims) == 1
        fields = dict(self.fields)
        fields[name] = Field("int", "affine", int(base), (int(step),))
        return Items(self.dims, fields, self.grid)

    def scaled_float(self, name: str, factor_field_of_other: np.ndarray) -> "Items":  # pragma: no cover
        raise NotImplementedError

    # ---- materialisation ---------------------------------------------------
    def column(self, name: str) -> np.ndarray:
        return self.fields[name].values(self.dims)

    def records(self) -> List[dict]:
        cols = {k: self.column(k) for k in self.fields}
        out = []
        for k in range(len(self)):
            out.append({name: (int(c[k]) if self.fields[name].kind == "int" else float(c[k]))
                        for name, c in cols.items()})
        return out


def as_items(itr) -> Items:
    if isinstance(itr, Items):
        return itr
    recs = list(itr)
    if len(recs) == 1 and len(recs[0]) == 0:
        return Items.single()
    return Items.from_records(recs)
