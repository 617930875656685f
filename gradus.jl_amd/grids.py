"""Grids.AdaptiveGrid (src/image-planes/adaptive-grid.jl): a 3 x 3 refinement tree over a rectangle, periodic in x if asked.

The reference's numbering throughout: cells are numbered from 1 in the order they were made (0 = "no cell"); the children
of a cell are indexed in column order,

     1 | 4 | 7
    ---+---+---
     2 | 5 | 8
    ---+---+---
     3 | 6 | 9

(x runs with the columns, y with the rows), neighbours are (top, right, bottom, left), `level` 1 is the first nine cells and
`locations` lists the child index a cell holds at every level down to its own.  Cells are stored as arrays, one row per
cell -- a sky reaches 10⁵-10⁶ cells -- and row i belongs to cell i: `grid.level[i]`, `grid.pos[i]` read as the reference's
`grid.cells[i].level`, `.pos`.  Row 0 is a null cell (level 0, NaN position, no children, no neighbours).
"""
from __future__ import annotations

import numpy as np

# (x, y) offsets of the nine children, in units of a child's width: CARDINAL_DIRECTIONS, adaptive-grid.jl:14-15
_DIRECTIONS = np.array([(x, y) for x in (-1, 0, 1) for y in (-1, 0, 1)], dtype=np.float64)
# the child indices facing top / right / down / left (adaptive-grid.jl:18-22), 0-based
_FACINGS = ((0, 3, 6), (6, 7, 8), (2, 5, 8), (0, 1, 2))
# direction a cell looks in -> the side of its neighbour that faces it, 0-based (FACING_LOOKUP, adaptive-grid.jl:25)
_FACING_LOOKUP = (2, 3, 0, 1)
# children's neighbours (adaptive-grid.jl:189-263): per child four entries (top, right, bottom, left); an entry k >= 0 is
# sibling k (0-based), -1 - d the PARENT's neighbour in direction d
_CHILD_NEIGHBOURS = np.array([
    (-1, 3, 1, -4), (0, 4, 2, -4), (1, 5, -3, -4),
    (-1, 6, 4, 0), (3, 7, 5, 1), (4, 8, -3, 2),
    (-1, -2, 7, 3), (6, -2, 8, 4), (7, -2, -3, 5),
], dtype=np.int64)


class AdaptiveGrid:
    """AdaptiveGrid(x1, x2, y1, y2; x_periodic = true), adaptive-grid.jl:44-121."""

    def __init__(self, x1, x2, y1, y2, x_periodic=True):
        x1, x2 = min(x1, x2), max(x1, x2)
        y1, y2 = min(y1, y2), max(y1, y2)
        self.limits = ((float(x1), float(x2)), (float(y1), float(y2)))
        self.x_periodic = bool(x_periodic)
        self.n = 0
        self._cap = 0
        self.pos = np.empty((0, 2))
        self.level = np.empty(0, dtype=np.int32)
        self.children = np.empty((0, 9), dtype=np.int64)       # 0 in column 0 = not refined
        self.neighbours = np.empty((0, 4), dtype=np.int64)
        self.parent = np.empty(0, dtype=np.int64)              # 0 = a top-level cell
        self.location = np.empty(0, dtype=np.int8)             # the child index (1 ... 9) the cell holds in its parent
        δ = np.array([x2 - x1, y2 - y1], dtype=np.float64)
        mid = δ / 2 + np.array([x1, y1], dtype=np.float64)
        self._reserve(9)
        self.pos[0] = np.nan
        for i in range(1, 10):
            self.pos[i] = mid + (δ / 3) * _DIRECTIONS[i - 1]
            self.level[i] = 1
            self.location[i] = i
        self.n = 9
        p = 1 if x_periodic else 0
        # (top, right, bottom, left), adaptive-grid.jl:108-118
        self.neighbours[1:10] = [(0, 4, 2, 7 * p), (1, 5, 3, 8 * p), (2, 6, 0, 9 * p),
                               (0, 7, 5, 1), (4, 8, 6, 2), (5, 9, 0, 3),
                               (0, 1 * p, 8, 4), (7, 2 * p, 9, 5), (8, 3 * p, 0, 6)]

    def __len__(self):
        return self.n

    def _reserve(self, extra):
        need = self.n + 1 + extra
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 1024)

        def grow(a, shape):
            b = np.zeros((cap,) + shape, dtype=a.dtype)
            k = min(self.n + 1, a.shape[0])
            b[:k] = a[:k]
            return b

        self.pos = grow(self.pos, (2,))
        self.level = grow(self.level, ())
        self.children = grow(self.children, (9,))
        self.neighbours = grow(self.neighbours, (4,))
        self.parent = grow(self.parent, ())
        self.location = grow(self.location, ())
        self._cap = cap

    # ---- the reference's accessors (cell indices count from 1) ----
    def extent(self):
        (x1, x2), (y1, y2) = self.limits
        return abs(x2 - x1), abs(y2 - y1)

    def has_children(self, cell_index):
        """bool, or a bool array for an index array"""
        return self.children[np.asarray(cell_index), 0] != 0

    def locations(self, cell_index):
        """the child indices this cell occupies at every level, top level first"""
        out = []
        i = int(cell_index)
        while i != 0:
            out.append(int(self.location[i]))
            i = int(self.parent[i])
        return out[::-1]

    def get_cell_width(self, cell_index):
        Δx, Δy = self.extent()
        f = 3.0 ** self.level[np.asarray(cell_index)]
        return Δx / f, Δy / f

    def leaves(self):
        """the indices of every cell without children, ascending"""
        return np.flatnonzero(self.children[1:self.n + 1, 0] == 0) + 1

    def refine_many(self, cell_indices):
        """refine! of each cell in turn, as one array operation per field.  Returns an (m, 9) array of the children's indices.
        (The children of cell k take the indices a loop of refine! calls in this order would give them; a child's neighbour
        outside its parent is the PARENT's neighbour, whether or not that one is refined: adaptive-grid.jl:189-263.)"""
        idx = np.asarray(cell_indices, dtype=np.int64).reshape(-1)
        m = idx.size
        if m == 0:
            return np.empty((0, 9), dtype=np.int64)
        if np.any(self.has_children(idx)):
            raise ValueError(f"{int(idx[np.flatnonzero(self.has_children(idx))[0]])} already refined")
        if np.unique(idx).size != m:
            raise ValueError("a cell is named twice")
        self._reserve(9 * m)
        first = self.n + 1 + 9 * np.arange(m, dtype=np.int64)
        kids = first[:, None] + np.arange(9, dtype=np.int64)[None, :]
        lev = self.level[idx] + 1
        Δx, Δy = self.extent()
        δ = np.stack([Δx / 3.0 ** lev, Δy / 3.0 ** lev], axis=-1)
        rows = kids.reshape(-1)
        self.pos[rows] = (self.pos[idx][:, None, :] + δ[:, None, :] * _DIRECTIONS[None, :, :]).reshape(-1, 2)
        self.level[rows] = np.repeat(lev, 9)
        self.parent[rows] = np.repeat(idx, 9)
        self.location[rows] = np.tile(np.arange(1, 10, dtype=np.int8), m)
        self.children[rows] = 0
        outer = self.neighbours[idx]                                          # (m, 4)
        code = _CHILD_NEIGHBOURS[None, :, :]                                  # (1, 9, 4)
        sib = first[:, None, None] + np.maximum(code, 0)
        par = np.take_along_axis(outer[:, None, :].repeat(9, axis=1), np.maximum(-1 - code, 0).repeat(m, axis=0), axis=2)
        self.neighbours[rows] = np.where(code >= 0, sib, par).reshape(-1, 4)
        self.children[idx] = kids
        self.n += 9 * m
        return kids

    def refine(self, cell_index):
        """refine!(grid, cell_index): split the cell into nine; returns the tuple of the children's indices"""
        return tuple(int(k) for k in self.refine_many([cell_index])[0])

    def _get_facing(self, out, cell_index, direction, level, locations):
        if not self.children[cell_index, 0]:
            out.append(cell_index)
            return
        kids = self.children[cell_index]
        own = int(self.level[cell_index])
        if own < level:
            # the neighbour is coarser than the asking cell was: follow the asking cell's own place (adaptive-grid.jl:311-314)
            loc = locations[own]
            position = (loc - 1) % 3 if direction % 2 == 1 else (loc - 1) // 3
            self._get_facing(out, int(kids[_FACINGS[direction][position]]), direction, level, locations)
        else:
            for k in _FACINGS[direction]:
                self._get_facing(out, int(kids[k]), direction, level, locations)

    def get_bordering(self, cell_index):
        """the leaves that touch the four sides of the cell (a list, in the reference's order: top, right, bottom, left)"""
        out = []
        cell_index = int(cell_index)
        level = int(self.level[cell_index])
        locations = self.locations(cell_index)
        for d in range(4):
            nb = int(self.neighbours[cell_index, d])
            if nb != 0:
                self._get_facing(out, nb, _FACING_LOOKUP[d], level, locations)
        return out

    def contains(self, cell_index, x, y):
        Δx, Δy = self.get_cell_width(cell_index)
        px, py = self.pos[cell_index]
        return bool((px - Δx / 2 < x) and (px + Δx / 2 > x) and (py - Δy / 2 < y) and (py + Δy / 2 > y))

    def _relative_location(self, cell_index, x, y):
        Δx, Δy = self.get_cell_width(cell_index)
        Δx, Δy = Δx / 6, Δy / 6
        px, py = self.pos[cell_index]
        xo = -1 if px - Δx > x else (1 if px + Δx < x else 0)
        yo = -1 if py - Δy > y else (1 if py + Δy < y else 0)
        return (1 + xo) * 3 + yo + 2

    def get_parent_index(self, x, y):
        """the most refined cell that contains (x, y); 0 outside the domain (or on a boundary between top-level cells)"""
        current = 0
        for i in range(1, 10):
            if self.contains(i, x, y):
                current = i
                break
        if current == 0:
            return 0
        while self.children[current, 0]:
            current = int(self.children[current, self._relative_location(current, x, y) - 1])
        return current

    def bordering_pairs(self):
        """every (leaf, bordering leaf) pair of find_need_refine (adaptive-sky.jl:130-152) as two index arrays, in the
        reference's visiting order: leaves ascending, each with its get_bordering list"""
        i1, i2 = [], []
        for c in self.leaves():
            b = self.get_bordering(int(c))
            i1.extend([int(c)] * len(b))
            i2.extend(b)
        return np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64)
