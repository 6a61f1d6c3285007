"""Surface mode, several lanes per query (k_tri_search_grid<L>, L = 2 or 4) under budget pressure.

The rows of a ring are dealt out to the L lanes of a query, and a lane takes further batches of rows in the same trip only
while its own range list has room: in rings >= 2 the lanes of one query drift apart.  A lane whose rows are empty is through
the ring (and settles on the cube bound) trips before a sibling with rows to list -- which may then go over its budget.  The
query must then go to the tree whichever of its lanes went over, and whenever.  These tests build the layouts that make this
happen, with the triangle grid's geometry under the test's control, and compare with the oracle's brute force over all
triangles, bit for bit.  The searches need a real MI355X (`pytest -m gpu`); the checks of the layouts' premises run anywhere."""
import numpy as np
import pytest

EYE = np.identity(4, dtype=np.float32)

# ---- the deterministic layout -------------------------------------------------------------------------------------------
# The host's cell size for triangles (build_tri_grid): h = OA_TRI_CELL (1.25) x the mean bounding-box diagonal, at least
# max_ext / 1023; cells from the vertices' bounding-box low corner, floor(ext / h) + 1 per axis.  Every triangle here is tiny
# (diagonal < 0.06) and the bounding box runs from (0, 0, 0) to (1023, Y, Z): h is exactly 1 and cell (i, j, k) is
# [i, i + 1) x [j, j + 1) x [k, k + 1).
#
# Offsets below are in cells, from the centre of the query's cell.  Ring 2 has 25 rows, kk = (dz + 2) 5 + (dy + 2); lane `sub`
# takes rows b0 + sub + L k, b0 advancing by RPL L (RPL = ceil(9 / L)) per batch; a lane takes another batch in the same trip
# only while n_seg + 2 RPL <= TRI_SEGS (10).
SEED = (1.15, 1.15, 1.15)          # ring 1 (corner cell): ~1.96 away; ring 1 finds it, the cube bound of ring 2 (2.5) settles on it
NEAR = (0.0, 1.55, 0.55)           # cell (0, 2, 1): row kk = 19 -- L = 2: lane 1, batch 2; L = 4: lane 3, batch 2.  ~1.62 away
CROWD_BOX = ((-0.4, 0.4), (2.0, 2.4), (1.0, 1.4))    # the same cell, farther than NEAR: more records than any lane's budget
N_CROWD = 60
# far (> 2.7) single triangles on lane 3's (L = 4) / lane 1's (L = 2) first-batch rows: kk = 3 (shell row), 7 and 11 (interior
# rows, both end cells).  L = 4: five ranges stop lane 3 after its first batch (5 + 6 > 10); L = 2: three ranges stop lane 1.
PADS = ((0.0, 1.4, -2.4), (2.4, 0.4, -1.4), (-2.4, 0.4, -1.4), (2.4, -1.4, 0.4), (-2.4, -1.4, 0.4))
QUERY_OFFSETS = ((0.0, 0.0, 0.0), (0.06, -0.05, 0.04), (-0.07, 0.03, -0.06))
SPACING = 12                       # cells between layouts along x: nothing of one layout within ring 3 of another's query
YZ = 24.0


def _tiny(c, s=0.02):
    """a small triangle in the plane x = c.x around c (diagonal ~ 2.8 s)"""
    c = np.asarray(c, np.float64)
    return np.array([c + [0.0, -s, -s], c + [0.0, s, -s], c + [0.0, 0.0, s]])


def _layout_mesh(signs_list=None, offsets=QUERY_OFFSETS):
    """Mirrored copies (every sign of x, y, z) of the layout above at every query offset, along x.  Returns (verts, tris,
    queries): float32 vertices, int32 triangles, float32 queries (one per copy)."""
    if signs_list is None:
        signs_list = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    rng = np.random.default_rng(1234)
    tris = [np.array([[0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.0, 0.02, 0.0]]),                 # the bounding box's corners
            np.array([[1023.0, YZ, YZ], [1022.98, YZ, YZ], [1023.0, YZ - 0.02, YZ]])]
    queries = []
    k = 0
    for sg in signs_list:
        sg = np.asarray(sg, np.float64)
        for off in offsets:
            centre = np.array([10 + SPACING * k, 10, 10], np.float64) + 0.5
            k += 1
            queries.append(centre + off)
            tris.append(_tiny(centre + sg * SEED))
            tris.append(_tiny(centre + sg * NEAR))
            for p in PADS:
                tris.append(_tiny(centre + sg * np.asarray(p)))
            lo = np.array([b[0] for b in CROWD_BOX]) + 0.02
            hi = np.array([b[1] for b in CROWD_BOX]) - 0.02
            for _ in range(N_CROWD):
                tris.append(_tiny(centre + sg * rng.uniform(lo, hi), s=0.01))
    assert 10 + SPACING * k < 1020
    v = np.concatenate(tris).astype(np.float32)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, t, np.array(queries, np.float32)


def _cell_geometry(v, t):
    """the host's triangle grid for this mesh (fp64, as build_tri_grid): h and the cells per axis"""
    tri = v[t].astype(np.float64)
    diag = np.sqrt(((tri.max(axis=1) - tri.min(axis=1)) ** 2).sum(axis=1))
    ext = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
    h = max(1.25 * diag.sum() / len(t), ext.max() / 1023.0)
    return h, np.floor(ext / h).astype(int) + 1


def test_layout_geometry_is_what_the_tests_assume(orc):
    """The deterministic layout's premises, checked on the CPU with the host's rules and the oracle: h = 1, lo = 0, the seed
    triangle is in the ring-1 corner cell, the nearest triangle is NEAR in the crowded ring-2 cell, everything else is farther
    than the seed."""
    v, t, q = _layout_mesh()
    h, n = _cell_geometry(v, t)
    assert h == 1.0 and tuple(n) == (1024, 25, 25) and v.min() == 0.0
    face, _, d2 = orc.nn_tri_brute(q, v, t)
    per = len(t) - 2
    per_copy = 2 + len(PADS) + N_CROWD
    assert per == per_copy * len(q)
    copy = (face - 2) // per_copy
    assert np.array_equal(copy, np.arange(len(q)))                    # every query's nearest is in its own copy
    assert np.all((face - 2) % per_copy == 1)                         # ... and it is NEAR
    seed_d2 = np.array([((q[k].astype(np.float64) - v[t[2 + per_copy * k]].mean(axis=0)) ** 2).sum() for k in range(len(q))])
    assert np.all(np.sqrt(d2) < 1.75) and np.all(np.sqrt(seed_d2) > 1.8) and np.all(np.sqrt(seed_d2) < 2.2)
    cells = np.floor(v[t].mean(axis=1)).astype(int)
    qc = np.floor(q).astype(int)
    for k in range(len(q)):
        rel = cells[2 + per_copy * k: 2 + per_copy * (k + 1)] - qc[k]
        assert np.abs(rel[0]).max() == 1                              # the seed: ring 1
        assert np.abs(rel[1:]).max(axis=1).min() == 2                 # NEAR, the pads, the crowd: ring 2
        assert np.abs(rel[1:]).max() == 2


def _search(v, t, q, env, monkeypatch, seeded, mx=EYE, seed_mx=None):
    from object_alignment_amd.engine import IcpEngine
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    with IcpEngine(0) as e:
        e.set_search_mode("grid")
        e.set_target_mesh(v, t)
        e.set_source(q)
        if seeded:
            e.set_matrices(EYE if seed_mx is None else seed_mx, EYE)
            e.make_pairs(1e6)                                 # plants the seeds (a bare nn_search does not)
        e.set_matrices(mx, EYE)
        idx, d2, _ = e.nn_search()
    return idx, d2


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_lane_settled_while_a_sibling_goes_over(orc, lanes, monkeypatch):
    """One lane of a query through ring 2 and settled on the seed's bound, a sibling still listing ring 2 goes over its budget
    on the crowded cell that holds the nearest triangle: the query goes to the tree -- index and float32 distance equal the
    brute force over all triangles, with and without the listed ranges of an over-budget batch dropped, unseeded and seeded."""
    v, t, q = _layout_mesh()
    face, _, rd2 = orc.nn_tri_brute(q, v, t)
    bad = {}
    for drop in ("0", "1"):
        for seeded in (False, True):
            env = {"OA_GRID_LANES": lanes, "OA_GRID_BUDGET": "16", "OA_GRID_BUDGET_MOVING": "1", "OA_TRI_DROP_OVER": drop}
            idx, d2 = _search(v, t, q, env, monkeypatch, seeded)
            bad[(drop, seeded)] = int(((idx != face) | (d2 != rd2)).sum())
    print("L = %s: mismatching queries of %d per (drop_over, seeded): %s" % (lanes, len(q), bad))
    assert not any(bad.values()), bad


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["2", "4"])
def test_loop_forms_on_the_layout(orc, lanes, monkeypatch):
    """The same layout through the ICP loop: its first iteration searches at the layout's pose, where a sibling lane goes over
    after lane 0 settled -- in the accumulating form (forced fast: the epilogue's `todo` ballot decides the hand-over) and in the
    plain ones (forced safe, adaptive, no fused accumulation).  The four leave the same bits, and the oracle's loop: K exact,
    M to 1e-9 (every pair is kept: thresh above every distance)."""
    from object_alignment_amd.engine import IcpEngine
    v, t, q = _layout_mesh()
    iters, thresh = 3, 10.0
    monkeypatch.setenv("OA_GRID_LANES", lanes)
    monkeypatch.setenv("OA_GRID_BUDGET", "16")
    monkeypatch.setenv("OA_GRID_BUDGET_MOVING", "1")
    out = {}
    for tag, env in (("fast", {"OA_GRID_PATH": "fast"}), ("safe", {"OA_GRID_PATH": "safe"}), ("adaptive", {}),
                     ("plain", {"OA_FUSED_ACC": "0"})):
        monkeypatch.delenv("OA_GRID_PATH", raising=False)
        monkeypatch.delenv("OA_FUSED_ACC", raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        with IcpEngine(0) as e:
            e.set_search_mode("grid")
            e.set_target_mesh(v, t)
            e.set_source(q, stride=1)
            e.set_matrices(EYE, EYE)
            out[tag] = e.run(iters=iters, thresh=thresh, target_d=1e-300, early_exit=False)
    ref = orc.icp_run(q, v, EYE, EYE, iters=iters, sample=1, thresh=thresh, target_d=1e-300, tris=t)
    for tag, r in out.items():
        assert np.array_equal(r.step_K, ref["step_K"]), tag
        assert np.abs(r.step_M - ref["step_M"]).max() < 1e-9, tag
    for tag in ("safe", "adaptive", "plain"):
        a, b = out["fast"], out[tag]
        assert np.array_equal(a.step_K, b.step_K), tag
        assert np.array_equal(a.step_M, b.step_M) and np.array_equal(a.matrix_world, b.matrix_world), tag


def _vertex_ppc(v):
    """OA_GRID_PPC that gives the vertex grid h = 1: the host sets h = (volume ppc / n_vertices)^(1/3) (build_grid)"""
    ext = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
    return len(v) / float(np.prod(ext))


def _vertex_cell_geometry(v, ppc):
    """the host's vertex grid for these vertices (fp64, as build_grid): h and the cells per axis"""
    ext = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
    h = (float(np.prod(ext)) * ppc / len(v)) ** (1.0 / 3.0)
    return h, np.floor(ext / h).astype(int) + 1


def test_vertex_layout_geometry_is_what_the_tests_assume(orc):
    """The vertex grid's premises on the same layout: h = 1 up to rounding, lo = 0, every query's nearest vertex is one of
    NEAR's, the seed's vertices are in the ring-1 corner cell, NEAR's and the crowd's in ring 2, and the crowded cell holds
    more vertices than any lane's budget."""
    v, t, q = _layout_mesh()
    h, n = _vertex_cell_geometry(v, _vertex_ppc(v))
    assert abs(h - 1.0) < 1e-12 and v.min() == 0.0
    assert tuple(n) in [(a, b, c) for a in (1023, 1024) for b in (24, 25) for c in (24, 25)], (h, n)
    idx, _ = orc.nn_brute(q, v)
    per_copy = 2 + len(PADS) + N_CROWD
    tri = idx // 3
    assert np.array_equal((tri - 2) // per_copy, np.arange(len(q))) and np.all((tri - 2) % per_copy == 1)
    cells = np.floor(v.astype(np.float64) / h).astype(int)
    qc = np.floor(q.astype(np.float64) / h).astype(int)
    for k in range(len(q)):
        rel = cells[3 * (2 + per_copy * k): 3 * (2 + per_copy * (k + 1))] - qc[k]
        ring = np.abs(rel).max(axis=1)
        assert np.all(ring[:3] == 1) and np.all(ring[3:] == 2)
        crowd = rel[3 * (2 + len(PADS)):]
        assert np.all(crowd == rel[3]) and len(crowd) > 16                 # NEAR's cell, 180 vertices
        assert np.all(rel[3:6] == rel[3])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["2", "4"])
def test_vertex_grid_lanes_stay_in_lockstep(orc, lanes, monkeypatch):
    """k_nn_search_grid<L> on the same layout's vertices, cells of the same size (OA_GRID_PPC set for h = 1), same budget: its
    lanes advance through a ring together, so a query's lanes agree on when a ring is done -- pinned here against the
    oracle's brute force, unseeded and seeded."""
    from object_alignment_amd.engine import IcpEngine
    v, t, q = _layout_mesh()
    ridx, rd2 = orc.nn_brute(q, v)
    monkeypatch.setenv("OA_GRID_LANES", lanes)
    monkeypatch.setenv("OA_GRID_BUDGET", "16")
    monkeypatch.setenv("OA_GRID_BUDGET_MOVING", "1")
    monkeypatch.setenv("OA_GRID_PPC", repr(_vertex_ppc(v)))
    with IcpEngine(0) as e:
        e.set_search_mode("grid")
        e.set_target(v)
        e.set_source(q)
        e.set_matrices(EYE, EYE)
        idx, d2, _ = e.nn_search()
        e.make_pairs(1e6)                                     # plants the seeds
        idx2, d22, _ = e.nn_search()
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2)
    assert np.array_equal(idx2, ridx) and np.array_equal(d22, rd2)


# ---- randomized meshes with uneven cell occupancy -----------------------------------------------------------------------
def _uneven_mesh(seed):
    """A sparse bumpy sheet, a second sheet a fraction of a cell above part of it, a few dense patches of thousands of tiny
    triangles in a handful of cells, slivers.  Returns (verts, tris, queries at 0.3 .. 3 h from the surface, h)."""
    rng = np.random.default_rng(seed)
    n = 28
    g = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    def sheet(z0, amp):
        return np.stack([X.ravel(), Y.ravel(), z0 + amp * np.sin(5 * X.ravel()) * np.cos(4 * Y.ravel())], 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel(); b = a + 1; c = a + n + 1; d = a + n + 2
    quad = np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, d], 1)])
    parts_v = [sheet(0.0, 0.04)]
    parts_t = [quad]
    nv = len(parts_v[0])
    upper = sheet(0.03, 0.04)                                          # the two-sheet case: over the x < 0.4 part
    keep = quad[(X.ravel()[quad] < 0.4).all(axis=1)]
    parts_v.append(upper); parts_t.append(keep + nv); nv += len(upper)
    for _ in range(4):                                                 # dense patches: tiny triangles in a small box on the sheet
        c0 = np.array([rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), 0.0])
        c0[2] = 0.04 * np.sin(5 * c0[0]) * np.cos(4 * c0[1])
        m = int(rng.integers(1500, 2500))
        cen = c0 + rng.uniform(-0.015, 0.015, size=(m, 3))
        pv = (cen[:, None, :] + rng.normal(scale=0.002, size=(m, 3, 3))).reshape(-1, 3)
        parts_v.append(pv); parts_t.append(np.arange(3 * m).reshape(-1, 3) + nv); nv += len(pv)
    m = 40                                                             # slivers: long and a hair wide, across several cells
    p0 = np.stack([rng.uniform(0, 1, m), rng.uniform(0, 1, m), rng.uniform(-0.05, 0.08, m)], 1)
    dirn = rng.normal(size=(m, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    sv = np.stack([p0, p0 + 0.15 * dirn, p0 + 0.075 * dirn + rng.normal(scale=1e-5, size=(m, 3))], 1).reshape(-1, 3)
    parts_v.append(sv); parts_t.append(np.arange(3 * m).reshape(-1, 3) + nv); nv += len(sv)
    v = np.concatenate(parts_v).astype(np.float32)
    t = np.concatenate(parts_t).astype(np.int32)
    h, _ = _cell_geometry(v, t)
    # queries: half over the dense patches and the sheets, half anywhere on the surface, 0.3 .. 3 h off it
    nq = 1500
    f = rng.integers(0, len(t), size=nq)
    w = rng.dirichlet([1.0, 1.0, 1.0], size=nq)
    p = (v[t[f]].astype(np.float64) * w[:, :, None]).sum(axis=1)
    dirq = rng.normal(size=(nq, 3)); dirq /= np.linalg.norm(dirq, axis=1, keepdims=True)
    q = (p + dirq * rng.uniform(0.3, 3.0, size=(nq, 1)) * h).astype(np.float32)
    return v, t, q, h


@pytest.fixture(scope="module")
def uneven():
    return _uneven_mesh(2024)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_uneven_occupancy_sweep(orc, uneven, lanes, monkeypatch):
    """budget x drop_over x shared / per-lane scan x unseeded / seeded (seeds from a nearby pose): every query bitwise the
    brute force over all triangles."""
    v, t, q, h = uneven
    face, _, rd2 = orc.nn_tri_brute(q, v, t)
    seed_mx = np.identity(4, dtype=np.float32)
    seed_mx[:3, 3] = np.float32(0.7 * h) * np.array([0.6, -0.48, 0.64], np.float32)   # stale seeds: 0.7 h away
    bad = {}
    for budget in ("8", "24", "64", None):
        for drop in ("0", "1"):
            for share in ("1", "0"):
                monkeypatch.delenv("OA_GRID_BUDGET", raising=False)
                env = {"OA_GRID_LANES": lanes, "OA_TRI_DROP_OVER": drop, "OA_TRI_SHARE": share}
                if budget is not None:
                    env["OA_GRID_BUDGET"] = budget
                for seeded in (False, True):
                    idx, d2 = _search(v, t, q, env, monkeypatch, seeded, seed_mx=seed_mx)
                    n_bad = int(((idx != face) | (d2 != rd2)).sum())
                    if n_bad:
                        bad[(budget, drop, share, seeded)] = n_bad
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["2", "4"])
def test_accumulating_form_under_budget_pressure(orc, uneven, lanes, monkeypatch):
    """The loop's grid search with its accumulating epilogue (whose `todo` ballot hands unsettled queries to the tree) and the
    other forms, on the uneven mesh with a small budget: forced fast, forced safe, adaptive and without the fused
    accumulation leave the same bits, and the oracle's loop (K exact, M to 1e-9)."""
    from object_alignment_amd import synth
    from object_alignment_amd.engine import IcpEngine
    v, t, q, h = uneven
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.02, -0.015, 0.01]), [0.01, -0.006, 0.004]).astype(np.float32)
    iters, thresh = 5, 0.5
    monkeypatch.setenv("OA_GRID_LANES", lanes)
    monkeypatch.setenv("OA_GRID_BUDGET", "8")
    out = {}
    for tag, env in (("safe", {"OA_GRID_PATH": "safe"}), ("fast", {"OA_GRID_PATH": "fast"}), ("adaptive", {}),
                     ("plain", {"OA_FUSED_ACC": "0"})):
        monkeypatch.delenv("OA_GRID_PATH", raising=False)
        monkeypatch.delenv("OA_FUSED_ACC", raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        with IcpEngine(0) as e:
            e.set_search_mode("grid")
            e.set_target_mesh(v, t)
            e.set_source(q, stride=1)
            e.set_matrices(mxa, EYE)
            out[tag] = e.run(iters=iters, thresh=thresh, target_d=1e-300, early_exit=False)
    for tag in ("fast", "adaptive", "plain"):
        a, b = out["safe"], out[tag]
        assert np.array_equal(a.step_K, b.step_K), tag
        assert np.array_equal(a.step_M, b.step_M) and np.array_equal(a.matrix_world, b.matrix_world), tag
    ref = orc.icp_run(q, v, mxa, EYE, iters=iters, sample=1, thresh=thresh, target_d=1e-300, tris=t)
    assert np.array_equal(out["safe"].step_K, ref["step_K"])
    assert np.abs(out["safe"].step_M - ref["step_M"]).max() < 1e-9
