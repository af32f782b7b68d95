"""What every device table of a scene must hold after rs_scene_set_triangles, restated in NumPy and Python record by record (helpers of
tests/test_refit_tables_host.py and tests/test_gpu_refit_tables.py).  An edit keeps the topology of every tree and the grid, so all of
it is parsed from a Snapshot of the tables taken BEFORE the first edit; the expected tables are then a function of the snapshot and the
edited vertices alone -- no table read back after the edit and no library call enters an expected value.  Everything is compared bit
for bit: the arithmetic is min / max on order-preserving integer keys, float32 subtraction and the double-precision predicate of
grid_box (rs_grid.h), all of which NumPy reproduces exactly."""
import numpy as np

from tests.geometry_edits import tree_children

EMPTY_BOX = (0xffffffff, 0x0000ffff, 0)          # lo = 65535 > hi = 0 on every axis: end records and padding records


# ---- keys: float32 <-> uint32 with the same order, -0 below +0 (rs_refit.h) ---------------------------------------------------------------
def refit_key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def refit_unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def refit_boxes_bits(vertices, order0):
    """The reference tree's boxes by boundingBoxId, (2n - 1, 6) float32, with the bits the header promises: a leaf is the min / max of
    its three vertices, an inner node of its two children (the record after it and that record's miss link), -0 below +0."""
    key = refit_key(np.asarray(vertices, np.float32).reshape(-1, 3, 3))
    o = np.asarray(order0, np.int32).reshape(-1, 3)
    lo, hi = np.zeros((len(o), 3), np.uint32), np.zeros((len(o), 3), np.uint32)
    for i in range(len(o) - 1, -1, -1):
        prim, box, _ = o[i]
        if prim >= 0:
            lo[box], hi[box] = key[prim].min(0), key[prim].max(0)
        else:
            a, b = o[i + 1, 1], o[o[i + 1, 2], 1]
            lo[box], hi[box] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
    return np.concatenate([refit_unkey(lo), refit_unkey(hi)], 1)


# ---- grid_box (rs_grid.h), the same double-precision expressions on arrays -------------------------------------------------------------
def grid_box(lo, hi, base, scale, margin):
    """lo, hi: (n, 3) float32 exact boxes.  Returns ((n, 3) uint32 box dwords, (n,) bool fits); rows that do not fit are left 0."""
    lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
    b, s = np.asarray(base, np.float32).astype(np.float64), np.asarray(scale, np.float32).astype(np.float64)
    margin = np.float64(margin)
    fits = ((lo >= np.float32(-3.4e38)) & (hi <= np.float32(3.4e38))).all(1)
    l, h = lo.astype(np.float64) - margin, hi.astype(np.float64) + margin
    with np.errstate(invalid="ignore", over="ignore"):
        lowest = np.floor((l - b) / s)
        highest = np.ceil((h - b) / s)
        for _ in range(64):                                  # while (b + lowest * s > lo - margin) lowest--;   multiply, then add
            move = fits[:, None] & (b + lowest * s > l)
            if not move.any():
                break
            lowest = lowest - move
        else:
            raise AssertionError("grid_box: the lower plane does not settle")
        for _ in range(64):
            move = fits[:, None] & (b + highest * s < h)
            if not move.any():
                break
            highest = highest + move
        else:
            raise AssertionError("grid_box: the upper plane does not settle")
    fits = fits & ((lowest >= 0) & (highest <= 65535)).all(1)
    ql = np.where(fits[:, None], lowest, 0).astype(np.int64).astype(np.uint32)
    qh = np.where(fits[:, None], highest, 0).astype(np.int64).astype(np.uint32)
    out = np.stack([ql[:, 0] | (ql[:, 1] << 16), ql[:, 2] | (qh[:, 0] << 16), qh[:, 1] | (qh[:, 2] << 16)], 1).astype(np.uint32)
    return out, fits


# ---- a pre-order array of grid-box records ----------------------------------------------------------------------------------------------
def leaf_slots(w, step):
    """The triangle slots of the leaf code w (sign bit set): ~w = first * 8 + count -> first, first + step, ..."""
    code = ~int(w)
    return [(code >> 3) + step * j for j in range(code & 7)]


def walk_preorder(w, step=1):
    """One binary tree in pre-order, every inner record followed by its two subtrees; w[i] < 0 marks a leaf.  An explicit stack of the
    open inner records [index, subtrees still to come].  Returns (parent, depth, end, slots): parent[i] (-1 at the root), the depth,
    end[i] = the index one past i's subtree, slots[i] = the triangle slots of a leaf (None at an inner record).
    ValueError: a second root, or records missing at the end."""
    n = len(w)
    parent, depth, end = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    slots = [None] * n
    stack = []
    for i in range(n):
        if i > 0 and not stack:
            raise ValueError("record %d starts a second root" % i)
        if stack:
            parent[i], depth[i] = stack[-1][0], len(stack)
            stack[-1][1] -= 1
        if int(w[i]) < 0:
            slots[i] = leaf_slots(w[i], step)
            end[i] = i + 1
            while stack and stack[-1][1] == 0:               # the subtree that ends here ends every open record it was the last part of
                end[stack.pop()[0]] = i + 1
        else:
            stack.append([i, 2])
    if n == 0 or stack:
        raise ValueError("the array ends inside a tree")
    return parent, depth, end, slots


def tree_length(w):
    """How many records from the start make one complete tree (a pre-order binary tree is complete where records == 2 * leaves - 1)."""
    leaves = 0
    for i in range(len(w)):
        leaves += int(w[i]) < 0
        if i + 1 == 2 * leaves - 1:
            return i + 1
    raise ValueError("no complete tree")


class GridTree:
    """One tree of occNodes / ordNodes as the snapshot holds it: records [first, first + count) of its table; prims[slot] = the primitive
    in a slot of its triangle array; step = -1 in a mirrored order.  Checks the snapshot's own consistency: miss links are the
    subtree ends, and the leaves list every slot once, ascending (descending in a mirrored order)."""

    def __init__(self, records, first, count, link_base, link_end, prims, step):
        self.first, self.count = first, count
        w = records["w"][first:first + count]
        self.parent, self.depth, end, slots = walk_preorder(w, step)
        for i in range(count):
            if w[i] >= 0:                                    # the miss link: the byte offset of the record after the subtree
                want = link_end if end[i] == count else link_base + int(end[i]) * 16
                assert int(w[i]) == want, (first, i, int(w[i]), want)
        self.leaves = np.array([i for i in range(count) if slots[i] is not None], np.int64)
        seq = [s for i in self.leaves for s in slots[i]]
        assert seq == list(range(len(prims)))[::step], "the leaves do not list the triangle array in order"
        self.width = max(len(slots[i]) for i in self.leaves)
        self.leaf_prims = np.full((len(self.leaves), self.width), -1, np.int64)
        for j, i in enumerate(self.leaves):
            self.leaf_prims[j, :len(slots[i])] = prims[slots[i]]

    def boxes(self, tri_lo, tri_hi):
        """The exact box of every record: the union of the boxes of the triangles in its span."""
        lo = np.full((self.count, 3), np.inf, np.float32)
        hi = np.full((self.count, 3), -np.inf, np.float32)
        for j in range(self.width):
            p = self.leaf_prims[:, j]
            m = p >= 0
            lo[self.leaves[m]] = np.minimum(lo[self.leaves[m]], tri_lo[p[m]])
            hi[self.leaves[m]] = np.maximum(hi[self.leaves[m]], tri_hi[p[m]])
        for d in range(int(self.depth.max()), 0, -1):        # children before parents
            i = np.nonzero(self.depth == d)[0]
            np.minimum.at(lo, self.parent[i], lo[i])
            np.maximum.at(hi, self.parent[i], hi[i])
        return lo, hi


class Snapshot:
    """The device tables, the grid and the threaded orders of a scene before its first edit, parsed."""

    def __init__(self, scene):
        from restir_amd import capi
        self.tables = {name: scene.debug_table(name).copy() for name in capi.SCENE_TABLES}
        self.grid = scene.debug_grid()
        self.nodes = scene.host_desc()["nodes"].copy()
        t = self.tables
        self.num_prims, self.bvh_size = len(t["vertices"]), self.nodes.shape[1]
        nn = self.bvh_size
        assert len(t["nodesAll"]) == 6 * nn + 1 and len(t["tris"]) == self.num_prims
        for k in range(6):                                   # the fused records carry the orders the host describes
            assert np.array_equal(t["nodesAll"]["primId"][k * nn:(k + 1) * nn], self.nodes[k][:, 0])
            assert np.array_equal(t["nodesAll"]["next"][k * nn:(k + 1) * nn], self.nodes[k][:, 2])
        _, leaves = tree_children(self.nodes[0])
        self.leaf_of = np.array([leaves[p] for p in range(self.num_prims)], np.int64)
        prim_of_leaf = np.full(nn, -1, np.int64)
        prim_of_leaf[self.leaf_of] = np.arange(self.num_prims)
        self.has_occ, self.has_ord = self.grid["occ_count"] > 0, self.grid["ord_stride"] > 0
        assert self.has_occ == (len(t["occNodes"]) > 0) == (len(t["occChain"]) > 0) == (len(t["occTris"]) > 0)
        assert self.has_ord == (len(t["ordNodes"]) > 0) == (len(t["ordTris"]) > 0)
        self.trees = []                                      # (table, GridTree)
        self.occ_prims, self.ord_prims = None, None
        if self.has_occ:
            no = self.grid["occ_count"]
            assert len(t["occNodes"]) == no + 1 and len(t["occChain"]) == nn
            self.occ_prims = prim_of_leaf[t["occTris"]["pad0"].astype(np.int64)]
            assert sorted(self.occ_prims) == list(range(self.num_prims))
            self.trees.append(("occNodes", GridTree(t["occNodes"], 0, no, 0, no * 16, self.occ_prims, 1)))
        if self.has_ord:
            per = self.grid["ord_stride"] // 16
            assert len(t["ordNodes"]) == 6 * per and len(t["ordTris"]) == 3 * self.num_prims
            self.ord_prims = t["ordTris"]["pad1"].astype(np.int64).reshape(3, self.num_prims)
            assert np.array_equal(t["ordTris"]["pad0"].astype(np.int64).reshape(3, -1), self.leaf_of[self.ord_prims])
            for k in range(6):
                first = k * per
                count = tree_length(t["ordNodes"]["w"][first:first + per - 1])
                end = (first + per - 1) * 16
                assert sorted(self.ord_prims[k >> 1]) == list(range(self.num_prims))
                self.trees.append(("ordNodes", GridTree(t["ordNodes"], first, count, first * 16, end, self.ord_prims[k >> 1], -1 if k & 1 else 1)))
                pad = np.arange(first + count, first + per)
                for r in t["ordNodes"][pad]:                 # padding records and the end record: empty, linked to the end record
                    assert tuple(r["box"]) == EMPTY_BOX and r["w"] == end

    def expected(self, vertices, normals):
        """{table: the array it must equal bit for bit} for a scene whose triangles are now `vertices`, `normals` ((n, 3, 3) float32)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3, 3)
        t, nn = self.tables, self.bvh_size
        out = {k: a.copy() for k, a in t.items()}            # what no kernel may write stays the snapshot's
        out["vertices"], out["normals"] = v.copy(), n.copy()

        def put(name, prims):
            out[name]["v0"], out[name]["e1"], out[name]["e2"] = v[prims, 0], v[prims, 1] - v[prims, 0], v[prims, 2] - v[prims, 0]
        put("tris", np.arange(self.num_prims))
        boxes = refit_boxes_bits(v, self.nodes[0])

        def put_boxes(name, rows, ids):
            a = out[name]
            a["min"][rows], a["maxx"][rows], a["maxy"][rows], a["maxz"][rows] = boxes[ids, :3], boxes[ids, 3], boxes[ids, 4], boxes[ids, 5]
        for k in range(6):
            put_boxes("nodesAll", slice(k * nn, (k + 1) * nn), self.nodes[k][:, 1])
        if self.has_occ:
            put("occTris", self.occ_prims)
            put_boxes("occChain", slice(0, nn), np.arange(nn))
        if self.has_ord:
            put("ordTris", self.ord_prims.reshape(-1))
        tri_lo, tri_hi = v.min(1), v.max(1)
        g = self.grid
        for name, tree in self.trees:
            lo, hi = tree.boxes(tri_lo, tri_hi)
            q, fits = grid_box(lo, hi, g["base"], g["scale"], g["margin"])
            assert fits.all(), "a vertex outside the grid's box was accepted"
            out[name]["box"][tree.first:tree.first + tree.count] = q
        return out


def table_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def first_difference(name, want, got):
    """A short description of the first record of `got` that differs from `want` (None when the tables are bitwise equal)."""
    if want.shape != got.shape or want.dtype != got.dtype:
        return "%s: shape %s %s, expected %s %s" % (name, got.shape, got.dtype, want.shape, want.dtype)
    if want.size == 0:
        return None
    rows = table_bytes(want).reshape(len(want), -1) != table_bytes(got).reshape(len(got), -1)
    bad = np.nonzero(rows.any(1))[0]
    if not len(bad):
        return None
    return "%s: %d of %d records differ, first at %d: expected %r, got %r" % (name, len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])


def assert_tables(want, scene, tag, only=None):
    """Every device table of `scene` equals `want` bit for bit."""
    from restir_amd import capi
    for name in (only or capi.SCENE_TABLES):
        d = first_difference(name, want[name], scene.debug_table(name))
        assert d is None, (tag, d)


def box_floats(nodes):
    """(n, 6) float32 min.xyz, max.xyz of nodesAll / occChain records."""
    return np.concatenate([nodes["min"], nodes["maxx"][:, None], nodes["maxy"][:, None], nodes["maxz"][:, None]], 1)
