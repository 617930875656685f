"""`AdaptiveGrid` (gradus.jl_amd/grids.py) against the reference's numbering (src/image-planes/adaptive-grid.jl): the
children's positions, `level` and `locations`, the nine neighbour tuples of a refined cell, the periodic seam, the
bordering leaves of a coarse cell next to a twice-refined one and the point lookup.  No GPU, no tracing."""
import numpy as np
import pytest

# adaptive-grid.jl:189-263, (top, right, bottom, left) of child k + 1; "c3" = sibling 3, "T/R/B/L" = the parent's neighbour there
NEIGHBOUR_TABLE = [
    ("T", "c4", "c2", "L"), ("c1", "c5", "c3", "L"), ("c2", "c6", "B", "L"),
    ("T", "c7", "c5", "c1"), ("c4", "c8", "c6", "c2"), ("c5", "c9", "B", "c3"),
    ("T", "R", "c8", "c4"), ("c7", "R", "c9", "c5"), ("c8", "R", "B", "c6"),
]


@pytest.fixture
def AdaptiveGrid():
    import gradus_jl_amd as G

    return G.AdaptiveGrid


def expected_neighbours(kids, outer):
    """the table above with the children's indices `kids` and the parent's neighbours `outer` = (top, right, bottom, left)"""
    side = dict(zip("TRBL", outer))
    return [tuple(kids[int(e[1:]) - 1] if e[0] == "c" else side[e] for e in row) for row in NEIGHBOUR_TABLE]


def test_top_level_cells_and_the_periodic_seam(AdaptiveGrid):
    g = AdaptiveGrid(0.0, 9.0, -3.0, 3.0)
    assert len(g) == 9 and g.extent() == (9.0, 6.0)
    # column order: x with the columns, y with the rows
    np.testing.assert_allclose(g.pos[1:10, 0], [1.5, 1.5, 1.5, 4.5, 4.5, 4.5, 7.5, 7.5, 7.5])
    np.testing.assert_allclose(g.pos[1:10, 1], [-2, 0, 2, -2, 0, 2, -2, 0, 2])
    assert list(g.level[1:10]) == [1] * 9 and [g.locations(i) for i in range(1, 10)] == [[i] for i in range(1, 10)]
    # (top, right, bottom, left), adaptive-grid.jl:108-118: cell 1 <-> 7 across the seam
    assert tuple(g.neighbours[1]) == (0, 4, 2, 7) and tuple(g.neighbours[7]) == (0, 1, 8, 4)
    assert tuple(g.neighbours[2]) == (1, 5, 3, 8) and tuple(g.neighbours[9]) == (8, 3, 0, 6)
    assert tuple(g.neighbours[5]) == (4, 8, 6, 2)
    h = AdaptiveGrid(0.0, 9.0, -3.0, 3.0, x_periodic=False)
    assert tuple(h.neighbours[1]) == (0, 4, 2, 0) and tuple(h.neighbours[7]) == (0, 0, 8, 4)
    # limits given the other way round are sorted (adaptive-grid.jl:86-89)
    assert AdaptiveGrid(9.0, 0.0, 3.0, -3.0).limits == g.limits


@pytest.mark.parametrize("cell", [5, 2, 1, 7], ids=["interior", "edge", "seam-left", "seam-right"])
def test_refine_places_children_and_wires_their_neighbours(AdaptiveGrid, cell):
    g = AdaptiveGrid(0.0, 9.0, -3.0, 3.0)
    outer = tuple(int(v) for v in g.neighbours[cell])
    centre = g.pos[cell].copy()
    kids = g.refine(cell)
    assert kids == tuple(range(10, 19)) and len(g) == 18
    assert g.has_children(cell) and not g.has_children(kids[0]) and tuple(g.children[cell]) == kids
    with pytest.raises(ValueError):
        g.refine(cell)
    # a child's width is 1/9 of the domain: offsets of one child width, column order
    for k, kid in enumerate(kids):
        np.testing.assert_allclose(g.pos[kid], centre + np.array([(k // 3 - 1) * 1.0, (k % 3 - 1) * (6.0 / 9.0)]), rtol=0, atol=1e-14)
        assert g.level[kid] == 2 and g.locations(kid) == [cell, k + 1]
        assert g.get_cell_width(kid) == (1.0, 6.0 / 9.0)
    assert [tuple(int(v) for v in g.neighbours[kid]) for kid in kids] == expected_neighbours(kids, outer)
    # the middle child sits where its parent does
    np.testing.assert_array_equal(g.pos[kids[4]], centre)
    # a second level below the first child
    grand = g.refine(kids[0])
    assert g.locations(grand[8]) == [cell, 1, 9] and g.level[grand[8]] == 3
    assert [tuple(int(v) for v in g.neighbours[q]) for q in grand] == expected_neighbours(grand, tuple(int(v) for v in g.neighbours[kids[0]]))


def test_refine_many_equals_a_loop_of_refine(AdaptiveGrid):
    a, b = AdaptiveGrid(-1.0, 1.0, -3.0, 3.0), AdaptiveGrid(-1.0, 1.0, -3.0, 3.0)
    a.refine_many([3, 1, 8])
    for c in (3, 1, 8):
        b.refine(c)
    a.refine_many(a.leaves())
    for c in b.leaves():
        b.refine(int(c))
    assert len(a) == len(b) == 9 + 27 + 9 * (6 + 27)
    n = len(a) + 1
    for name in ("pos", "level", "children", "neighbours", "parent", "location"):
        np.testing.assert_array_equal(getattr(a, name)[:n], getattr(b, name)[:n], err_msg=name)


def test_bordering_of_a_coarse_cell_next_to_a_twice_refined_one(AdaptiveGrid):
    g = AdaptiveGrid(0.0, 9.0, 0.0, 9.0, x_periodic=False)
    k5 = g.refine(5)             # the centre cell ...
    k52 = g.refine(k5[1])        # ... its left-middle child (location 2: x -, y middle) once more
    k54 = g.refine(k5[3])        # ... and its top-middle child (location 4)
    # cell 2 is the coarse cell to the LEFT of cell 5: it faces the left column of 5 (children 1, 2, 3), of which child 2 is
    # refined and shows its own left column; in the reference's order top, right, bottom, left
    assert g.get_bordering(2) == [1, k5[0], k52[0], k52[1], k52[2], k5[2], 3]
    # cell 4 is above cell 5: the top row of 5 (children 1, 4, 7), child 4 refined -> its top row
    assert g.get_bordering(4) == [7, k5[0], k54[0], k54[3], k54[6], k5[6], 1]
    # a fine cell next to a coarse one sees the coarse cell once: the grandchild at the left edge of child 2 looks at cell 2
    assert g.get_bordering(k52[1]) == [k52[0], k52[4], k52[2], 2]
    # the middle child of 5 between the two refined ones: the bottom row of child 4 above it, the right column of child 2 beside it
    assert g.get_bordering(k5[4]) == [k54[2], k54[5], k54[8], k5[7], k5[5], k52[6], k52[7], k52[8]]
    # every cell named is a leaf
    for c in g.leaves():
        assert not any(g.has_children(b) for b in g.get_bordering(int(c)))


def test_bordering_of_a_child_follows_its_own_place_in_a_coarser_refined_neighbour(AdaptiveGrid):
    """adaptive-grid.jl:311-314: a level-2 cell whose (inherited) neighbour is a level-1 cell refined twice sees only the part
    of that neighbour's facing side that lies against it"""
    g = AdaptiveGrid(0.0, 9.0, 0.0, 9.0, x_periodic=False)
    k5, k2 = g.refine(5), g.refine(2)
    k2_8 = g.refine(k2[7])       # child 8 of cell 2: right column, middle row -- it touches child 2 of cell 5
    # child 2 of cell 5 (left column, middle) looks left at cell 2 (level 1, refined): position "middle" of its right column is
    # child 8, refined -> that one's right column
    left = [c for c in g.get_bordering(k5[1]) if c not in (k5[0], k5[4], k5[2])]
    assert left == [k2_8[6], k2_8[7], k2_8[8]]


def test_contains_and_get_parent_index_find_the_leaf(AdaptiveGrid):
    g = AdaptiveGrid(-1.0, 1.0, -np.pi, np.pi)
    g.refine_many(g.leaves())
    g.refine_many([11, 40, 77])
    g.refine_many([g.children[40][4]])
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(-1, 1, 1000), rng.uniform(-np.pi, np.pi, 1000)], axis=-1)
    leaves = g.leaves()
    wx, wy = g.get_cell_width(leaves)
    lo = g.pos[leaves] - np.stack([wx, wy], axis=-1) / 2
    hi = g.pos[leaves] + np.stack([wx, wy], axis=-1) / 2
    for x, y in pts:
        inside = np.flatnonzero((lo[:, 0] < x) & (x < hi[:, 0]) & (lo[:, 1] < y) & (y < hi[:, 1]))
        assert inside.size == 1
        got = g.get_parent_index(x, y)
        assert got == leaves[inside[0]] and g.contains(got, x, y)
    for x, y in ((1.5, 0.0), (-1.0001, 0.0), (0.0, 3.2), (0.3, -4.0)):
        assert g.get_parent_index(x, y) == 0
