"""MI355X-native ICP alignment engine (hot path of patmo141/object_alignment)."""


def estimate_normals(xyz, k=16, orient="none", orient_point=None, device=0):
    """PCA normals of ANY point cloud (the source's included: the normal-angle test needs source normals too), estimated on
    the GPU: (normals float32 (n, 3), curvature float32 (n,)).  Opens a context of its own on `device`, uploads xyz as its
    target, estimates from every point's k nearest neighbours (IcpEngine.estimate_target_normals) and closes."""
    from .engine import IcpEngine
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        return eng.estimate_target_normals(k=k, orient=orient, orient_point=orient_point, install=False)
