"""What an upload forgets ("Who owns device memory"): a context that has held other targets and sources before computes,
reports and holds exactly what a fresh context given only the current target, source and settings does.

One engine walks through cloud A, mesh B, cloud C, mesh B again and a second source, with every per-target and per-source
feature on (normal test, estimated target normals, kept FPFH descriptors, the mesh's pseudo-normals through a signed deviation
call, reciprocal check, estimated trim, boundary rejection, a robust loss with its scale from the residuals).  After every upload
a fresh engine gets the same target, source and settings; the two must agree bit for bit on the loop's result and history, and
exactly on every statistic that describes the resident target.  The memory test: after cloud -> mesh the context holds no more
device memory than a context that only ever saw the mesh, and everything returns when the last context closes.
"""
import gc

import numpy as np
import pytest

from object_alignment_amd import synth

pytestmark = pytest.mark.gpu

STATS = ("grid_cells", "tri_grid_cells", "tri_grid_entries", "n_tris", "surface", "safe_radii", "tri_ring", "target_normals",
         "target_features", "mesh_pseudonormals", "target_boundary", "boundary_vertices", "boundary_edges")
ITERS, THRESH = 5, 0.5
POOL_SLACK = 8 << 20                   # what tests/test_gpu_multi_device.py grants to runtime-internal pools


def _pose():
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.05, -0.04, 0.06]), [0.02, -0.015, 0.02])
    return mxa, np.identity(4, dtype=np.float32)


def _settings(e):
    """the settings that survive uploads: given once, to the walking engine at its creation and to every fresh one"""
    e.set_reciprocal(True, 1.0)
    e.set_trim("auto")
    e.set_reject_boundary(True)
    e.set_robust("huber", 1.4826 * 1.345)
    e.set_robust_auto(0.5, 1e-4)


def _run(e, target, source):
    """what belongs to the resident pair, then the loop: the same calls in the same order on both engines"""
    mxa, mxb = _pose()
    e.set_matrices(mxa, mxb)
    if target[0] == "cloud":
        e.estimate_target_normals(k=16, orient="away", install=True)
        e.target_fpfh(k=16, keep=True)
    else:
        e.deviation(thresh=THRESH, signed=True, outputs=("signed_d",))     # builds the mesh's pseudo-normals
    e.set_normals(source[1], None, 60.0)
    res = e.run(iters=ITERS, thresh=THRESH, early_exit=False)
    return res, {name: e.stat(name) for name in STATS}


def _upload_target(e, target):
    if target[0] == "cloud":
        e.set_target(target[1])
    else:
        e.set_target_mesh(target[1], target[2])


def test_a_context_with_a_past_equals_a_fresh_one_after_every_upload():
    from object_alignment_amd.engine import IcpEngine
    cloud_a = ("cloud", synth.bunny_surface(3000, 0.0))
    cloud_c = ("cloud", synth.bunny_surface(1500, 0.3))
    mesh_b = ("mesh",) + tuple(synth.icosphere_mesh(2))
    source_1 = synth.bunny_surface_with_normals(1500, 0.5)
    source_2 = synth.bunny_surface_with_normals(3000, 0.7)
    steps = [("target", cloud_a), ("target", mesh_b), ("target", cloud_c), ("target", mesh_b), ("source", source_2)]
    with IcpEngine(0) as walker:
        _settings(walker)
        target, source = None, source_1
        walker.set_source(source[0])
        for n, (what, data) in enumerate(steps):
            if what == "target":
                target = data
                _upload_target(walker, target)
            else:
                source = data
                walker.set_source(source[0])
            got, got_stats = _run(walker, target, source)
            with IcpEngine(0) as fresh:
                _settings(fresh)
                _upload_target(fresh, target)
                fresh.set_source(source[0])
                ref, ref_stats = _run(fresh, target, source)
            where = "after upload %d (%s, a %s target of %d vertices, %d source points)" % (n, what, target[0], len(target[1]), len(source[0]))
            print(where, "walker", got_stats, "K", got.step_K.tolist(), "fresh", ref_stats, "K", ref.step_K.tolist())
            assert got.iters_done == ref.iters_done == ITERS, where
            assert got_stats == ref_stats, where
            assert np.array_equal(got.step_K, ref.step_K), where
            assert got.matrix_world.tobytes() == ref.matrix_world.tobytes(), where
            assert got.step_M.tobytes() == ref.step_M.tobytes() and got.step_new.tobytes() == ref.step_new.tobytes(), where
            # the features were really on: the stats of the fresh engine say so
            if target[0] == "cloud":
                assert ref_stats["surface"] == 0 and ref_stats["grid_cells"] > 0 and ref_stats["target_normals"] == 1 and ref_stats["target_features"] == 1, where
                assert ref_stats["n_tris"] == 0 and ref_stats["tri_grid_cells"] == 0 and ref_stats["mesh_pseudonormals"] == 0, where
            else:
                assert ref_stats["surface"] == 1 and ref_stats["n_tris"] == len(target[2]) and ref_stats["mesh_pseudonormals"] == 1, where
                assert ref_stats["grid_cells"] == 0 and ref_stats["target_normals"] == 0 and ref_stats["target_features"] == 0, where
            assert ref_stats["target_boundary"] == 1, where


def _held(torch, free0):
    from object_alignment_amd import _capi
    _capi.load().oa_release_cached_memory()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info(0)[0]


def test_a_mesh_after_a_cloud_holds_what_a_mesh_alone_holds():
    import torch
    from object_alignment_amd import _capi
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.functions.general import close_default_engines
    torch.cuda.init()
    close_default_engines()                                    # engines other tests left alive keep the cache alive
    gc.collect()
    _capi.load().oa_release_cached_memory()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    # 400 000 points, the size of test_device_memory_returns_after_destroy: the cloud's blocks are then larger than the 2 MiB
    # fragments the HIP runtime sub-allocates small blocks from and keeps pooled until the context closes.  (Measured at 100 000
    # points: 12 MiB held after the mesh upload against 2 MiB for the mesh alone, before this test's change and after it alike --
    # all of it the runtime's pool.  At 400 000: 64 MiB held before the change, the old cloud's vertex grid; 4 MiB after it.)
    cloud = synth.bunny_surface(400_000, 0.0)
    verts, tris = synth.icosphere_mesh(2)
    source = synth.bunny_surface(3000, 0.5)
    with IcpEngine(0) as e:
        e.set_target_mesh(verts, tris)
        e.set_source(source)
        mesh_only = _held(torch, free0)
    with IcpEngine(0) as e:
        e.set_target(cloud)
        e.set_source(source)
        with_cloud = _held(torch, free0)
        e.set_target_mesh(verts, tris)
        after = _held(torch, free0)
        print("device bytes held: mesh only %d, cloud %d, mesh after the cloud %d" % (mesh_only, with_cloud, after))
        assert with_cloud - mesh_only > POOL_SLACK             # the cloud's images and indices are visible above the allowance
        assert after <= mesh_only + POOL_SLACK, (mesh_only, with_cloud, after)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free0 - free1 <= POOL_SLACK, (free0, free1)         # back to the baseline
