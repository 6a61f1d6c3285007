"""MI355X-native ICP alignment engine (hot path of patmo141/object_alignment)."""


def estimate_normals(xyz, k=16, orient="none", orient_point=None, device=0, radius=None):
    """PCA normals of ANY point cloud (the source's included: the normal-angle test needs source normals too), estimated on
    the GPU: (normals float32 (n, 3), curvature float32 (n,)).  Opens a context of its own on `device`, uploads xyz as its
    target, estimates from every point's k nearest neighbours (IcpEngine.estimate_target_normals) and closes.  radius: only
    neighbours within it count (xyz's own units; IcpEngine.set_neighbor_radius); None: the k nearest however far."""
    from .engine import IcpEngine, _radius_arg
    if radius is not None:
        radius = _radius_arg(radius, "estimate_normals")
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        return eng.estimate_target_normals(k=k, orient=orient, orient_point=orient_point, install=False, radius=radius)


def cloud_spacing(xyz, device=0):
    """The point spacing of ANY cloud, measured on the GPU: {"mean", "std"} of the distance from every point to the nearest other
    point, "n_finite" and "n_nonfinite" (IcpEngine.target_spacing) -- the scale a neighbour radius, a voxel edge or a clustering
    eps is a multiple of.  Opens a context of its own on `device`, uploads xyz as its target and closes."""
    import numpy as np
    from .engine import IcpEngine
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or len(xyz) < 1:
        raise ValueError("cloud_spacing: xyz must be (n >= 1, 3), got shape %s" % (xyz.shape,))
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        return eng.target_spacing()


def orient_normals(xyz, normals, k=8, max_dist=0.0, seed="away", point=None, device=0):
    """One consistent sign for the normals of ANY point cloud, on the GPU: signs handed along the minimum spanning forest of the
    k-nearest graph (Hoppe et al. 1992) -- (normals float32 (n, 3), flipped uint8 (n,), component int32 (n,), report dict;
    IcpEngine.orient_target_normals says how to read them).  Opens a context of its own on `device`, uploads xyz as its target
    and closes."""
    import numpy as np
    from .engine import IcpEngine, _orient_args
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or len(xyz) < 2:
        raise ValueError("orient_normals: xyz must be (n >= 2, 3), got shape %s" % (xyz.shape,))
    if normals is None:
        raise ValueError("orient_normals: normals must be (n, 3) numbers, got None")
    k, max_dist, seed, point, normals = _orient_args(k, max_dist, seed, point, normals, n=len(xyz), name="orient_normals")
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        return eng.orient_target_normals(k=k, max_dist=max_dist, seed=seed, point=point, normals=normals, install=False)


def remove_outliers(xyz, method="statistical", k=16, std_ratio=2.0, radius=0.0, min_neighbors=8, count_cap=0, device=0):
    """Stray points of ANY point cloud, found on the GPU (IcpEngine.target_outliers says how): a dict with "xyz" (the kept points,
    float32, in the caller's order), "index" (their indices, ascending), "keep" uint8 (n,), "score" or "count", and "report".
    Opens a context of its own on `device`, uploads xyz as its target and closes."""
    import numpy as np
    from .engine import IcpEngine, _outlier_args
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or len(xyz) < 2:
        raise ValueError("remove_outliers: xyz must be (n >= 2, 3), got shape %s" % (xyz.shape,))
    _outlier_args(method, k, std_ratio, radius, min_neighbors, count_cap, n=len(xyz), name="remove_outliers")
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        out = eng.target_outliers(method=method, k=k, std_ratio=std_ratio, radius=radius, min_neighbors=min_neighbors,
                                  count_cap=count_cap, apply=False)
    out["xyz"] = xyz[out["index"]]
    return out


def cluster_dbscan(xyz, eps, min_points=8, keep="clustered", min_size=0, device=0):
    """The parts of ANY point cloud, by DBSCAN on the GPU (IcpEngine.target_clusters says how): a dict with "label" int32 (n,) (-1:
    noise), "sizes" int32 (n_clusters,), "keep" uint8 (n,), "index" (the kept points' indices, ascending), "xyz" (the kept points,
    float32, in the caller's order) and "report".  Opens a context of its own on `device`, uploads xyz as its target and closes."""
    import numpy as np
    from .engine import IcpEngine, _cluster_args
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or len(xyz) < 1:
        raise ValueError("cluster_dbscan: xyz must be (n >= 1, 3), got shape %s" % (xyz.shape,))
    _cluster_args(eps, min_points, keep, min_size, name="cluster_dbscan")
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        out = eng.target_clusters(eps, min_points=min_points, keep=keep, min_size=min_size, apply=False)
    out["xyz"] = xyz[out["index"]]
    return out


def fpfh(xyz, normals=None, k=16, normal_k=16, device=0, radius=None):
    """Fast Point Feature Histograms of ANY point cloud (the source's included), computed on the GPU: (n, 33) float32, an
    all-zero row meaning "no descriptor".  Opens a context of its own on `device` and uploads xyz as its target; without
    `normals` (n, 3) they are estimated from every point's normal_k nearest neighbours, oriented away from the centroid.
    radius: only neighbours within it count, for the descriptors and for normals estimated here (xyz's own units;
    IcpEngine.set_neighbor_radius); None: the k nearest however far."""
    import numpy as np
    from .engine import IcpEngine, _fpfh_k, _radius_arg
    k = _fpfh_k(k)
    if radius is not None:
        radius = _radius_arg(radius, "fpfh")
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or len(xyz) < 4:
        raise ValueError("fpfh: xyz must be (n >= 4, 3), got shape %s" % (xyz.shape,))
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != xyz.shape:
            raise ValueError("fpfh: %s normals for %s points" % (normals.shape, xyz.shape))
    elif int(normal_k) != normal_k or not 3 <= int(normal_k) <= 64:
        raise ValueError("fpfh: normal_k = %r outside 3 .. 64" % (normal_k,))
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        if normals is None:
            eng.estimate_target_normals(k=min(int(normal_k), len(xyz)), orient="away", install=True, radius=radius)
        else:
            eng.set_target_normals(normals)
        return eng.target_fpfh(k=min(k, len(xyz)), keep=False, radius=radius)


def mesh_boundary(verts, tris, device=0):
    """The boundary of ANY triangle mesh, found on the GPU: (vertex_mask uint8 (n_verts,), edge_mask uint8 (n_tris,)) -- bit j of
    edge_mask[t] says that local edge j of triangle t (ab, bc, ca) belongs to exactly one triangle, vertex_mask marks the ends of
    such edges (IcpEngine.target_boundary).  Opens a context of its own on `device` and uploads the mesh as its target."""
    from .engine import IcpEngine
    with IcpEngine(int(device)) as eng:
        eng.set_target_mesh(verts, tris)
        return eng.target_boundary()


def cloud_boundary(xyz, normals, k=16, angle_deg=90.0, device=0, radius=None):
    """The rim of ANY point cloud by the angle criterion, found on the GPU: vertex_mask uint8 (n,), 1 where the largest angular
    gap between a point's k nearest neighbours, seen in its tangent plane, exceeds angle_deg (IcpEngine.target_boundary).
    normals: (n, 3), or "estimate" (PCA normals from every point's k nearest neighbours).  Opens a context of its own on
    `device` and uploads xyz as its target.  radius: only neighbours within it count, for the criterion and for normals estimated
    here (xyz's own units; IcpEngine.set_neighbor_radius) -- the k nearest no longer reach across a hole narrower than their
    spread; None: the k nearest however far."""
    from .engine import IcpEngine, _radius_arg
    if isinstance(normals, str) and normals != "estimate":
        raise ValueError("cloud_boundary: normals %r (an array of normals, or 'estimate')" % (normals,))
    if radius is not None:
        radius = _radius_arg(radius, "cloud_boundary")
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        if isinstance(normals, str):
            eng.estimate_target_normals(k=int(k), orient="none", install=True, radius=radius)
        else:
            eng.set_target_normals(normals)
        return eng.target_boundary(k=k, angle_deg=angle_deg, radius=radius)[0]


def voxel_downsample(xyz, voxel, normals=None, origin=None, device=0):
    """Voxel-grid downsample of ANY point cloud on the GPU: one row per occupied cell of edge `voxel` -- the members' mean, the
    normalised sum of their normals, their number and the index of the member nearest to the mean (a dict: xyz, normals or
    None, count, rep, report; IcpEngine.voxel_downsample).  Opens a context of its own on `device`."""
    from .engine import IcpEngine, _voxel_args
    xyz, normals, origin = _voxel_args(xyz, voxel, normals, origin)
    with IcpEngine(int(device)) as eng:
        return eng.voxel_downsample(xyz, voxel, normals=normals, origin=origin)


def normal_space_sample(normals, m, grid=8, unoriented=False, seed=0, device=0):
    """Normal-space sampling of ANY cloud's normals on the GPU: m points drawn evenly across the buckets of a cube map of the
    normals, so that small features keep their say (a dict: idx -- a vlist --, bin, report; IcpEngine.normal_space_sample).  Opens
    a context of its own on `device`."""
    from .engine import IcpEngine, _sample_args
    normals, m, grid, unoriented, seed = _sample_args(normals, m, grid, unoriented, seed)
    with IcpEngine(int(device)) as eng:
        return eng.normal_space_sample(normals, m, grid=grid, unoriented=bool(unoriented), seed=seed)


def stability(xyz, normals, idx=None, device=0):
    """Which rigid motions a selection of ANY cloud resists under the point-to-plane metric: the 6 x 6 constraint matrix of the
    points idx lists (None: all), its eigenvalues and eigenvectors, rank and condition number (a dict; IcpEngine.stability says
    how to read it).  Opens a context of its own on `device`."""
    from .engine import IcpEngine, _stability_args
    xyz, normals, idx = _stability_args(xyz, normals, idx)
    with IcpEngine(int(device)) as eng:
        return eng.stability(xyz, normals, idx=idx)


def deviation(source_xyz, target_xyz, target_tris=None, mx_align=None, mx_base=None, target_normals=None, device=0, **kw):
    """The deviation report of a source against a target at given matrices (identity when None): signed per-point distances and
    fit statistics (IcpEngine.deviation; **kw are its arguments).  target_tris: the target is a mesh and the sign comes from its
    pseudo-normals; else target_normals (one per target vertex) sign a point-cloud target.  Opens a context of its own on
    `device`."""
    import numpy as np
    from .engine import IcpEngine, _deviation_args
    _deviation_args(**kw)
    eye = np.eye(4, dtype=np.float32)
    with IcpEngine(int(device)) as eng:
        if target_tris is not None:
            eng.set_target_mesh(target_xyz, target_tris)
        else:
            eng.set_target(target_xyz)
            if target_normals is not None:
                eng.set_target_normals(target_normals)
        eng.set_source(source_xyz)
        eng.set_matrices(eye if mx_align is None else mx_align, eye if mx_base is None else mx_base)
        return eng.deviation(**kw)
