"""The texts of the refusals that the pair filters (oa_set_reciprocal, oa_set_trim, oa_set_reject_boundary) and the metrics that read
normals (plane, GICP, symmetric) give before a loop, oa_make_pairs or the split-phase loop starts: one table of (settings, call) ->
(error code, the whole message).  Every one of these calls is refused before a kernel is launched, and the context stays usable.

The host layer composes several of the messages from a noun ("the %s metric", the caller's name); the table holds them whole, as
a caller reads them.

Not in the table: the PLANE_MAX_BLOCKS capacity refusal of the three metrics ("the %s metric takes shards of up to 8388608 points
(this one: %d): use more shards"), which takes a selection of more than 8 388 608 points -- test_gpu_capacity_texts uploads one.
"""
import numpy as np
import pytest

from object_alignment_amd import synth
from test_boundary import half_cloud
from test_reciprocal import THRESH, usual_pose

STATE, BAD_ARG, CAPACITY = "OA_E_STATE", "OA_E_BAD_ARG", "OA_E_CAPACITY"
NOUN = {"plane": "plane", "gicp": "GICP", "symmetric": "symmetric"}

RIGID = "the %s metric solves for a rigid step: with_scale must be 0 (or call oa_set_metric(ctx, OA_METRIC_POINT))"
TARGET_NORMALS = ("the %s metric needs target normals: call oa_set_target_normals (or oa_set_normals) after oa_set_target, or upload a mesh with "
                  "oa_set_target_mesh")
SOURCE_NORMALS = "the %s metric needs source normals: call oa_set_source_normals (or oa_set_normals) after oa_set_source"
GICP_FIXED_SCALE = ("the GICP metric takes a robust loss with a fixed scale only: call oa_set_robust_auto(ctx, 0, 0) (or oa_set_metric(ctx, "
                    "OA_METRIC_PLANE))")
SHARD = {
    "recip": "%s with the reciprocal check on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call "
             "oa_set_reciprocal(ctx, 0, 1))",
    "trim": "%s with oa_set_trim on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call "
            "oa_set_trim(ctx, 0, 0, 2))",
    "bnd": "%s with oa_set_reject_boundary on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call "
           "oa_set_reject_boundary(ctx, 0, 16, 90))",
}
ONE_DEVICE = {
    "recip": "%s: the reciprocal check needs every selected source point on one device: it runs on a single-device context through oa_run / "
             "oa_iterate / oa_make_pairs (call oa_set_reciprocal(ctx, 0, 1) for this path)",
    "trim": "%s: oa_set_trim needs every selected source point's residual on one device: it runs on a single-device context through oa_run / "
            "oa_iterate / oa_make_pairs (call oa_set_trim(ctx, 0, 0, 2) for this path)",
    "bnd": "%s: oa_set_reject_boundary runs on a single-device context through oa_run / oa_iterate / oa_make_pairs (call "
           "oa_set_reject_boundary(ctx, 0, 16, 90) for this path)",
    "metric": "%s: the %s metric runs on a single-device context through oa_run / oa_iterate (call oa_set_metric(ctx, OA_METRIC_POINT) for this "
              "path)",
    "auto": "%s: a robust scale estimated from the residuals runs on a single-device context through oa_run / oa_iterate (call "
            "oa_set_robust_auto(ctx, 0, 0) for this path)",
}
ON = {"recip": dict(recip=True), "trim": dict(trim=0.5), "bnd": dict(bnd=True)}
AUTO = dict(loss="tukey", auto=0.5)
# who the text names -> the calls that go that way
CALLS = {
    "a loop": [("run", lambda e: e.run(iters=5, thresh=THRESH)), ("iterate", lambda e: e.iterate(thresh=THRESH))],
    "oa_make_pairs": [("make_pairs", lambda e: e.make_pairs(THRESH))],
}


def table():
    """[(label, settings, call, code, message)] for a single-device context"""
    rows = []
    loop = CALLS["a loop"][0][1]
    for metric, noun in NOUN.items():                               # begin_loop: what the three metrics ask for, in the order of the checks
        rows.append((metric + " with_scale", dict(metric=metric), lambda e: e.run(iters=5, thresh=THRESH, with_scale=True), BAD_ARG, RIGID % noun))
        rows.append((metric + " no target normals", dict(metric=metric, tn=False), loop, STATE, TARGET_NORMALS % noun))
        # (with_scale is looked at first, the target's normals before the source's)
        rows.append((metric + " with_scale, no normals at all", dict(metric=metric, tn=False, sn=False),
                     lambda e: e.run(iters=5, thresh=THRESH, with_scale=True), BAD_ARG, RIGID % noun))
        rows.append((metric + " no normals at all", dict(metric=metric, tn=False, sn=False), loop, STATE, TARGET_NORMALS % noun))
        if metric != "plane":
            rows.append((metric + " no source normals", dict(metric=metric, sn=False), loop, STATE, SOURCE_NORMALS % noun))
    rows.append(("gicp estimated scale", dict(metric="gicp", **AUTO), loop, STATE, GICP_FIXED_SCALE))
    rows.append(("gicp estimated scale, no source normals", dict(metric="gicp", sn=False, **AUTO), loop, STATE, SOURCE_NORMALS % "GICP"))
    for who, calls in CALLS.items():                                # a shard: the three filters, and who wins when two are on
        for name, call in calls:
            for f in ("recip", "trim", "bnd"):
                rows.append(("shard %s %s" % (f, name), dict(shard=True, **ON[f]), call, STATE, SHARD[f] % who))
            rows.append(("shard trim+bnd %s" % name, dict(shard=True, trim=0.5, bnd=True), call, STATE, SHARD["trim"] % who))
            rows.append(("shard recip+trim %s" % name, dict(shard=True, recip=True, trim=0.5), call, STATE, SHARD["recip"] % who))
            rows.append(("shard all three %s" % name, dict(shard=True, recip=True, trim=0.5, bnd=True), call, STATE, SHARD["recip"] % who))
    begin = lambda e: e.run_begin(iters=5, thresh=THRESH)           # the split-phase loop: refuse_wide_row's seven
    for f in ("recip", "trim", "bnd"):
        rows.append(("run_begin " + f, ON[f], begin, STATE, ONE_DEVICE[f] % "oa_run_begin"))
    for metric, noun in NOUN.items():
        rows.append(("run_begin " + metric, dict(metric=metric), begin, STATE, ONE_DEVICE["metric"] % ("oa_run_begin", noun)))
    rows.append(("run_begin estimated scale", AUTO, begin, STATE, ONE_DEVICE["auto"] % "oa_run_begin"))
    rows.append(("run_begin trim+bnd", dict(trim=0.5, bnd=True), begin, STATE, ONE_DEVICE["trim"] % "oa_run_begin"))
    rows.append(("run_begin recip+trim", dict(recip=True, trim=0.5), begin, STATE, ONE_DEVICE["recip"] % "oa_run_begin"))
    rows.append(("run_begin bnd + plane", dict(bnd=True, metric="plane"), begin, STATE, ONE_DEVICE["bnd"] % "oa_run_begin"))
    rows.append(("run_begin plane + estimated scale", dict(metric="plane", **AUTO), begin, STATE, ONE_DEVICE["metric"] % ("oa_run_begin", "plane")))
    return rows


def stage(e, d, metric="point", loss="none", auto=0.0, recip=False, trim=0.0, bnd=False, shard=False, tn=True, sn=True):
    e.set_metric(metric)
    e.set_robust(loss, 0.05 if loss != "none" else 0.0)
    e.set_robust_auto(auto, 1e-3 if auto else 0.0)
    e.set_reciprocal(recip)
    e.set_trim(trim)
    e.set_reject_boundary(bnd)
    e.set_target(d["tgt"])
    if tn:
        e.set_target_normals(d["tn"])
    e.set_source(d["src"], stride=1, shard_index=0, shard_count=2 if shard else 1)
    if sn:
        e.set_source_normals(d["sn"])
    e.set_matrices(d["mxa"], d["mxb"])


def refused(label, call, e, code, msg):
    from object_alignment_amd import _capi
    with pytest.raises(_capi.OaError) as ei:
        call(e)
    assert (ei.value.code, ei.value.msg) == (getattr(_capi, code), msg), label


def clouds():
    mxa, mxb = usual_pose()
    src, sn = synth.bunny_surface_with_normals(3000, 0.5)
    tgt, tn = half_cloud()
    return dict(src=np.asarray(src, np.float32), sn=np.asarray(sn, np.float32), tgt=tgt, tn=tn, mxa=mxa, mxb=mxb)


@pytest.mark.gpu
def test_gpu_refusal_texts():
    from object_alignment_amd.engine import IcpEngine
    d = clouds()

    def plain_loop(e):
        stage(e, d)
        r = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5
        return r

    with IcpEngine(0) as e:
        want = plain_loop(e)
        for label, settings, call, code, msg in table():
            stage(e, d, **settings)
            refused(label, call, e, code, msg)
        assert np.array_equal(plain_loop(e).step_K, want.step_K)   # every refusal left the context usable
    with IcpEngine(devices=[0, 0]) as m:
        want_m = plain_loop(m)
        who = "oa_make_pairs on a multi-device context"
        for f in ("recip", "trim", "bnd"):
            stage(m, d, **ON[f])
            refused("multi make_pairs " + f, lambda m_: m_.make_pairs(THRESH), m, STATE, ONE_DEVICE[f] % who)
        stage(m, d, trim=0.5, bnd=True)
        refused("multi make_pairs trim+bnd", lambda m_: m_.make_pairs(THRESH), m, STATE, ONE_DEVICE["trim"] % who)
        stage(m, d, recip=True, trim=0.5)
        refused("multi make_pairs recip+trim", lambda m_: m_.make_pairs(THRESH), m, STATE, ONE_DEVICE["recip"] % who)
        assert np.array_equal(plain_loop(m).step_K, want_m.step_K)


@pytest.mark.gpu
def test_gpu_capacity_texts():
    """One point more than PLANE_MAX_BLOCKS * PLANE_THREADS = 8 388 608 selected: the last of begin_loop's checks for the three metrics.
    (The size is the refusal's own threshold: no smaller selection reaches the text.)"""
    from object_alignment_amd.engine import IcpEngine
    d = clouds()
    n = 16384 * 512 + 1
    big = np.zeros((n, 3), np.float32)
    big[:, 2] = 1.0                                                 # (every point the same, its normal +z: nothing ever reads them)
    with IcpEngine(0) as e:
        e.set_target(d["tgt"])
        e.set_target_normals(d["tn"])
        e.set_source(big, stride=1)
        e.set_source_normals(big)
        e.set_matrices(d["mxa"], d["mxb"])
        for metric, noun in NOUN.items():
            e.set_metric(metric)
            refused(metric + " capacity", lambda e_: e_.run(iters=5, thresh=THRESH), e, CAPACITY,
                    "the %s metric takes shards of up to 8388608 points (this one: %d): use more shards" % (noun, n))
        stage(e, d)
        r = e.run(iters=5, thresh=THRESH, target_d=0.01, early_exit=False)
        assert r.iters_done == 5
