"""What makes a node array a BVH of a mesh in the reference's layout, checked without any builder: the tree is walked from its root
and every property is recomputed from the triangles themselves with exact comparisons (node bounds are min / max of float32
corners, so nothing is rounded). Shared by tests/test_bvh_edges_host.py (host builder) and tests/test_bvh_device.py (GPU builder)."""
import numpy as np

MAX_DEPTH = 64


def check_bvh(arrays, root, tri_first, tri_count):
    """`arrays`: Scene.numpy(). Asserts, for the mesh whose BVH is rooted at node `root` and whose triangles are
    [tri_first, tri_first + tri_count):
      - an interior node (triCount == 0) has the consecutive pair index, index + 1 as children, and the pair of the k-th interior
        node in left-first pre-order sits at root + 1 + 2k (the reference allocates a pair when it splits a node and finishes the
        left subtree first), so the mesh's nodes are exactly [root, root + node count);
      - a node's triangle range is its left child's followed by its right child's, the root's is the whole mesh, so every
        triangle lies in exactly one leaf;
      - every node's six bounds equal the min / max over the corners of the triangles of its range (as floats: -0 == +0);
      - no leaf is deeper than 64.
    Returns (node count, max leaf depth, min leaf depth, max leaf size): Scene.last_bvh_stats() of that mesh."""
    nodes = arrays["bvhNodes"].view(np.uint32).reshape(-1, 8)
    bounds = nodes[:, :6].view(np.float32)
    tris = arrays["triangles"].view(np.uint32).reshape(len(arrays["triangles"]), -1)[:, :3]
    pts = arrays["triPoints"].view(np.float32).reshape(len(arrays["triPoints"]), -1)[:, :3]
    assert tri_first + tri_count <= len(tris) and root < len(nodes)
    corners = pts[tris[tri_first:tri_first + tri_count].astype(np.int64)]       # [tri_count, 3 corners, xyz]
    tmin, tmax = corners.min(axis=1), corners.max(axis=1)

    covered = np.zeros(tri_count, np.int64)
    seen = set()
    interior = 0
    leaf_depths, leaf_sizes = [], []

    def visit(v, depth):
        """The triangle range (first, count) below node v."""
        nonlocal interior
        assert v < len(nodes), f"node {v} lies outside the node array"
        assert v not in seen, f"node {v} is reached twice"
        seen.add(v)
        index, count = int(nodes[v, 6]), int(nodes[v, 7])
        if count:
            assert depth <= MAX_DEPTH, f"leaf {v} at depth {depth}"
            first = index - tri_first
            assert 0 <= first and first + count <= tri_count, f"leaf {v}: triangles [{index}, {index + count}) outside the mesh"
            covered[first:first + count] += 1
            leaf_depths.append(depth)
            leaf_sizes.append(count)
        else:
            assert depth < MAX_DEPTH, f"interior node {v} at depth {depth}"
            assert index == root + 1 + 2 * interior, f"node {v}: children at {index}, the reference numbers them {root + 1 + 2 * interior}"
            interior += 1
            lf, lc = visit(index, depth + 1)
            rf, rc = visit(index + 1, depth + 1)
            assert lc > 0 and rc > 0 and rf == lf + lc, f"node {v}: children's ranges ({lf}, {lc}) and ({rf}, {rc}) are not consecutive"
            first, count = lf, lc + rc
        lo, hi = tmin[first:first + count].min(axis=0), tmax[first:first + count].max(axis=0)
        want = np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], np.float32)
        assert np.array_equal(bounds[v], want), f"node {v}: bounds {bounds[v].tolist()}, its triangles span {want.tolist()}"
        return first, count

    assert visit(root, 0) == (0, tri_count), "the root's range is not the whole mesh"
    assert (covered == 1).all(), f"triangles not in exactly one leaf: {np.flatnonzero(covered != 1)[:5].tolist()}"
    assert seen == set(range(root, root + len(seen))), "the mesh's nodes are not one contiguous block"
    return len(seen), max(leaf_depths), min(leaf_depths), max(leaf_sizes)


def stats_tuple(stats):
    """Scene.last_bvh_stats() in check_bvh's order."""
    return stats["nodeCount"], stats["maxDepth"], stats["minDepth"], stats["maxTri"]
