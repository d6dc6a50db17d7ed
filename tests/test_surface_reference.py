"""The surface restatement (tests/surface_ref.py) on analytic fields: closed, consistently oriented meshes with the
right topology and volume, normals that agree with the faces, and a case table whose every triangle points out."""
import numpy as np
import pytest

import surface_ref as S

F32 = np.float32


def _grid(n=24, lo=-1.2, hi=1.2):
    origin = np.full(3, lo, F32)
    spacing = np.full(3, F32((hi - lo) / (n - 1)), F32)
    ax = S.axes(origin, spacing, (n, n, n))
    z, y, x = np.meshgrid(ax[2].astype(np.float64), ax[1].astype(np.float64), ax[0].astype(np.float64), indexing="ij")
    return origin, spacing, (n, n, n), x, y, z


def _gauss(q2, s2):
    """exp(-q2 / (2 s2)) and d/dq2 of it"""
    f = np.exp(-q2 / (2 * s2))
    return f, -f / (2 * s2)


def ball(c=(0.0, 0.0, 0.0), r=0.8):
    origin, spacing, dims, x, y, z = _grid()
    s2 = 0.25
    dx, dy, dz = x - c[0], y - c[1], z - c[2]
    f, df = _gauss(dx * dx + dy * dy + dz * dz, s2)
    g = np.stack([2 * dx * df, 2 * dy * df, 2 * dz * df], -1)
    iso = np.exp(-r * r / (2 * s2))
    return origin, spacing, dims, f, g, iso, 4.0 / 3.0 * np.pi * r ** 3


def two_balls():
    origin, spacing, dims, x, y, z = _grid()
    s2, r = 0.04, 0.4
    fs, gs = 0.0, 0.0
    for cx in (-0.6, 0.6):
        dx = x - cx
        f, df = _gauss(dx * dx + y * y + z * z, s2)
        fs = fs + f
        gs = gs + np.stack([2 * dx * df, 2 * y * df, 2 * z * df], -1)
    iso = np.exp(-r * r / (2 * s2))
    return origin, spacing, dims, fs, gs, iso, 2 * 4.0 / 3.0 * np.pi * r ** 3


def torus(R=0.7, r=0.3):
    origin, spacing, dims, x, y, z = _grid()
    s2 = 0.05
    rho_xy = np.sqrt(x * x + y * y)
    q = rho_xy - R
    f, df = _gauss(q * q + z * z, s2)
    safe = np.where(rho_xy > 0, rho_xy, 1.0)
    g = np.stack([2 * q * x / safe * df, 2 * q * y / safe * df, 2 * z * df], -1)
    iso = np.exp(-r * r / (2 * s2))
    return origin, spacing, dims, f, g, iso, 2 * np.pi ** 2 * R * r * r


@pytest.mark.parametrize("field,chi", [(ball, 2), (two_balls, 4), (torus, 0)], ids=["ball", "two-balls", "torus"])
def test_analytic_fields_give_closed_outward_meshes(field, chi):
    origin, spacing, dims, f, g, iso, vol = field()
    xyz, nrm, tri = S.extract(f.astype(F32), g.astype(F32), origin, spacing, dims, F32(iso))
    assert len(tri) > 100
    assert xyz.dtype == np.float32 and nrm.dtype == np.float32 and tri.dtype == np.uint32
    assert tri.max() < len(xyz) and len(np.unique(tri)) == len(xyz)  # every vertex is used
    assert S.closed_and_oriented(tri, len(xyz))
    assert S.euler_characteristic(tri, len(xyz)) == chi
    v = S.signed_volume(xyz, tri)
    assert v > 0 and abs(v - vol) / vol < 0.05, (v, vol)
    fn = S.face_normals(xyz, tri)
    area = np.linalg.norm(fn, axis=1)
    big = area > 1e-6 * area.max()
    mean_n = nrm.astype(np.float64)[tri.astype(np.int64)].sum(1)
    assert np.all(np.einsum("ij,ij->i", fn[big], mean_n[big]) > 0)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)


def test_a_field_without_normals_gives_the_same_mesh():
    origin, spacing, dims, f, g, iso, _ = ball()
    a = S.extract(f.astype(F32), g.astype(F32), origin, spacing, dims, F32(iso))
    b = S.extract(f.astype(F32), None, origin, spacing, dims, F32(iso))
    assert b[1] is None
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2], b[2])


def test_every_case_of_every_tet_points_from_inside_to_outside():
    corner = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.float64)
    for t, q in enumerate(S.TETS):
        p = corner[list(q)]
        det = np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]]))
        assert (det < 0) == S.FLIP[t], t
        for case in range(1, 15):
            ins = [(case >> b) & 1 for b in range(4)]
            mid = {e: 0.5 * (p[u] + p[v]) for e, (u, v) in enumerate(S.LOCAL_EDGES)}
            out_dir = p[[b for b in range(4) if not ins[b]]].mean(0) - p[[b for b in range(4) if ins[b]]].mean(0)
            tris = S.CASES[case]
            assert len(tris) == (2 if sum(ins) == 2 else 1)
            for tri in tris:
                for e in tri:  # only crossed edges
                    u, v = S.LOCAL_EDGES[e]
                    assert ins[u] != ins[v], (t, case, tri)
                a, b, c = (mid[e] for e in tri)
                n = np.cross(b - a, c - a) * (-1 if S.FLIP[t] else 1)
                assert np.dot(n, out_dir) > 0, (t, case, tri)


def test_a_grid_with_a_node_inside_on_the_boundary_is_open():
    origin, spacing, dims, f, g, iso, _ = ball(c=(1.0, 0.0, 0.0))
    xyz, _, tri = S.extract(f.astype(F32), None, origin, spacing, dims, F32(iso))
    assert len(tri) > 0 and not S.closed_and_oriented(tri, len(xyz))
