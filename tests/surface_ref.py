"""numpy restatement of ws_extract_surface (include/wsfluid.h): marching tetrahedra on a sampled density grid, in float32
with every operation rounded, in the header's order -- vertices by node then edge type, triangles by cube, tet, table
entry.  It takes the grid field (what ws_sample_density_grid returns) and gives (vertices, normals, triangles), to be
compared with the library bit for bit.  Also the mesh checks the tests share: closedness, Euler characteristic,
signed volume."""
import numpy as np

F32 = np.float32

# the six tets of a cube along its 0-7 diagonal (corner c at (c & 1, c >> 1 & 1, c >> 2 & 1)); tets 1, 2, 5 are
# negatively oriented, so their triangles are written (v0 v2 v1)
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
FLIP = (False, True, True, False, False, True)
# local edges of a tet (q0 q1 q2 q3)
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# case (bit k = q_k inside) -> triangles as local edges, for a positively oriented tet (the header's table)
CASES = {
    1: ((0, 1, 2),), 2: ((0, 4, 3),), 4: ((1, 3, 5),), 8: ((2, 5, 4),),
    14: ((0, 2, 1),), 13: ((0, 3, 4),), 11: ((1, 5, 3),), 7: ((2, 4, 5),),
    3: ((1, 2, 4), (1, 4, 3)), 12: ((1, 3, 4), (1, 4, 2)),
    5: ((2, 0, 3), (2, 3, 5)), 10: ((3, 0, 2), (3, 2, 5)),
    9: ((0, 1, 5), (0, 5, 4)), 6: ((0, 4, 5), (0, 5, 1)),
}


def _offset(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def axes(origin, spacing, dims):
    """Node coordinates per axis: fl(origin + fl(i * spacing))."""
    o = np.asarray(origin, F32).reshape(3)
    s = np.asarray(spacing, F32).reshape(3)
    return [(o[a] + np.arange(int(dims[a]), dtype=F32) * s[a]).astype(F32) for a in range(3)]


def extract(rho, grad, origin, spacing, dims, iso):
    """rho (nz, ny, nx) float32, grad (nz, ny, nx, 3) float32 or None -> (xyz (V, 3) f32, normals (V, 3) f32 or None,
    triangles (T, 3) uint32)."""
    nx, ny, nz = (int(v) for v in dims)
    iso = F32(iso)
    r = np.ascontiguousarray(rho, F32).reshape(-1)
    n_nodes = nx * ny * nz
    node = np.arange(n_nodes, dtype=np.int64)
    i, j, k = node % nx, (node // nx) % ny, node // (nx * ny)
    inside = r >= iso
    # crossed forward edges, (node, d - 1)
    crossed = np.zeros((n_nodes, 7), bool)
    for d in range(1, 8):
        dx, dy, dz = _offset(d)
        ok = (i + dx < nx) & (j + dy < ny) & (k + dz < nz)
        m = node[ok] + dx + dy * nx + dz * nx * ny
        crossed[ok, d - 1] = inside[ok] != inside[m]
    # vertices in the order node, then d
    vid = (np.cumsum(crossed.reshape(-1), dtype=np.int64) - 1).reshape(n_nodes, 7)
    a, dm1 = np.nonzero(crossed)
    d = dm1 + 1
    dx, dy, dz = d & 1, (d >> 1) & 1, (d >> 2) & 1
    b = a + dx + dy * nx + dz * nx * ny
    ax = axes(origin, spacing, dims)
    pa = np.stack([ax[0][i[a]], ax[1][j[a]], ax[2][k[a]]], 1)
    pb = np.stack([ax[0][i[a] + dx], ax[1][j[a] + dy], ax[2][k[a] + dz]], 1)
    ra, rb = r[a], r[b]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        t = ((iso - ra) / (rb - ra)).astype(F32)
        xyz = (pa + t[:, None] * (pb - pa)).astype(F32)
        nrm = None
        if grad is not None:
            g = np.ascontiguousarray(grad, F32).reshape(-1, 3)
            ga, gb = g[a], g[b]
            gi = (ga + t[:, None] * (gb - ga)).astype(F32)
            gg = ((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2]).astype(F32)
            length = np.sqrt(gg).astype(F32)
            q = (-gi / length[:, None]).astype(F32)
            nrm = np.where((gg != 0)[:, None], q, F32(0)).astype(F32)
    # triangles: cubes in linear order of corner 0, then tet, then table entry
    cube = node[(i < nx - 1) & (j < ny - 1) & (k < nz - 1)]
    corner_node = [cube + cx + cy * nx + cz * nx * ny for cx, cy, cz in map(_offset, range(8))]
    tab = np.zeros((16, 2, 3), np.int64)
    ntab = np.zeros(16, np.int64)
    for s, tris in CASES.items():
        ntab[s] = len(tris)
        for q, e in enumerate(tris):
            tab[s, q] = e
    per_tet, per_ok = [], []
    rows = np.arange(len(cube))[:, None, None]
    for t_, q in enumerate(TETS):
        case = sum(inside[corner_node[c]].astype(np.int64) << bit for bit, c in enumerate(q))
        edge_vid = np.stack([vid[corner_node[q[u] & q[v]], (q[u] ^ q[v]) - 1] for u, v in LOCAL_EDGES], 1)
        tri = edge_vid[rows, tab[case]]  # (cubes, 2, 3)
        if FLIP[t_]:
            tri = tri[:, :, [0, 2, 1]]
        per_tet.append(tri)
        per_ok.append(np.arange(2)[None, :] < ntab[case][:, None])
    tri = np.stack(per_tet, 1).reshape(-1, 3)
    ok = np.stack(per_ok, 1).reshape(-1)
    tri = tri[ok]
    assert tri.size == 0 or tri.min() >= 0
    return xyz, nrm, tri.astype(np.uint32)


# ---- mesh checks ------------------------------------------------------------------------------------------------------
def directed_edges(tri):
    t = tri.astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def closed_and_oriented(tri, n_vertices):
    """Every directed edge appears exactly once and its reverse exactly once (a closed, consistently oriented mesh)."""
    e = directed_edges(tri)
    key = e[:, 0] * n_vertices + e[:, 1]
    rev = e[:, 1] * n_vertices + e[:, 0]
    if len(np.unique(key)) != len(key):
        return False
    return np.array_equal(np.sort(key), np.sort(rev))


def euler_characteristic(tri, n_vertices):
    e = directed_edges(tri)
    und = np.unique(np.sort(e, 1), axis=0)
    return int(n_vertices) - len(und) + len(tri)


def signed_volume(xyz, tri):
    p = xyz.astype(np.float64)[tri.astype(np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def face_normals(xyz, tri):
    p = xyz.astype(np.float64)[tri.astype(np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def components(tri, n_vertices):
    """Connected components of the mesh (by shared vertices): a label per vertex."""
    parent = np.arange(n_vertices)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in tri.astype(np.int64):
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    return np.array([find(v) for v in range(n_vertices)])
