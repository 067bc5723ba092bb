"""The _host entry points share one staging routine and one ctx buffer (rt_device.hip: staged, hostStageBuf; DESIGN.md,
"Staging"). One Renderer on the Cornell scene runs them back to back through the numpy paths of engine.py, so that the buffer
grows and is reused at smaller sizes by calls with other part lists:

  1 query_closest, 65 rays with tmax      5 build_sample_map from a moments plane
  2 denoise, 64 x 48                      6 temporal_accumulate, 64 x 48 (frame and moments)
  3 query_nearest, 1 point                7 query_occluded, 65 rays without tmax
  4 query_radiance, 65 rays with ids,     8 query_closest, 257 rays
    progressive

Each result must equal, bit for bit, the same call made as the only _host call of a fresh Renderer: a wrong offset, an in/out part
that is not uploaded, an absent part that is not NULL, or anything a call takes from what used the buffer before shows as a
difference. A refused _host call in between (tmax given to the radiance query) changes nothing either. The inputs (a frame, its
first-hit planes, the rays) are made once, on a renderer of their own, by calls that stage nothing."""
import ctypes as C

import numpy as np
import pytest

from ray_tracer_amd import _capi, engine

from util import bits, cornell_scene

W, H = 64, 48


def _words(x):
    """A result as one uint32 array: what bit-for-bit equality is taken on."""
    if isinstance(x, dict):
        return np.concatenate([_words(x[k]) for k in sorted(x)])
    if isinstance(x, tuple):
        return np.concatenate([_words(v) for v in x])
    a = np.ascontiguousarray(x)
    return bits(a.astype(np.uint32) if a.dtype == np.bool_ else a).reshape(-1)


def _fresh():
    r = engine.Renderer(0)
    r.upload_scene(cornell_scene(True))
    return r


@pytest.fixture(scope="module")
def calls(built):
    """name -> the call on a renderer, in the order of the sequence; the inputs are shared and never written."""
    src = _fresh()
    try:
        pc = engine.push_constants(W, H, singleRender=1, sampleLimit=2, bounceLimit=3)
        frame = src.render(pc, W, H)
        aovs = src.render_aovs(pc, W, H)
    finally:
        src.close()
    dirs = np.ascontiguousarray(aovs["ray_dir"].reshape(-1, 3)[::11][:257], np.float32)
    origins = np.ascontiguousarray(np.repeat(np.array(list(pc.camInfo.pos), np.float32)[None], 257, 0))
    depth = aovs["depth"].reshape(-1)[::11][:65]
    tmax = (depth * np.where(np.arange(65) % 2 == 0, np.float32(0.5), np.float32(2.0))).astype(np.float32)   # every other hit out of reach
    ids = (np.arange(65, dtype=np.uint32) * np.uint32(7) + np.uint32(3))
    prev = np.random.default_rng(3).uniform(0, 1, (65, 4)).astype(np.float32)
    point = np.array([[0.1, 0.2, -0.3]], np.float32)

    def temporal(r):
        return r.temporal_accumulate(pc, frame, aovs, moments=True)

    ref = _fresh()
    try:
        moments = temporal(ref)[1]
    finally:
        ref.close()
    for a in (frame, dirs, origins, tmax, ids, prev, point, moments, *aovs.values()):
        a.setflags(write=False)
    return pc, [
        ("query_closest 65 tmax", lambda r: engine.hits_to_numpy(r.query_closest(origins[:65], dirs[:65], tmax))),
        ("denoise", lambda r: r.denoise(frame, aovs)),
        ("query_nearest 1", lambda r: engine.nearest_to_numpy(r.query_nearest(point))),
        ("query_radiance 65 ids progressive", lambda r: r.query_radiance(origins[:65], dirs[:65], samples=2, bounces=3, ids=ids, progressive=True, frame=1, out=prev)),
        ("build_sample_map", lambda r: r.build_sample_map(moments)),
        ("temporal_accumulate", temporal),
        ("query_occluded 65", lambda r: r.query_occluded(origins[:65], dirs[:65])),
        ("query_closest 257", lambda r: engine.hits_to_numpy(r.query_closest(origins, dirs))),
    ]


@pytest.fixture(scope="module")
def alone(calls):
    """Each call as the only _host call of a fresh renderer."""
    want = {}
    for name, call in calls[1]:
        r = _fresh()
        try:
            want[name] = _words(call(r))
        finally:
            r.close()
    return want


@pytest.mark.gpu
def test_host_forms_back_to_back_equal_each_alone(calls, alone):
    r = _fresh()
    try:
        for name, call in calls[1]:
            got = _words(call(r))
            assert got.shape == alone[name].shape and np.array_equal(got, alone[name]), \
                f"{name}: {int((got != alone[name]).sum())} of {got.size} words differ from the call alone on a fresh renderer"
    finally:
        r.close()
    # (the results are results: not all zero words)
    assert all(w.any() for w in alone.values())


@pytest.mark.gpu
def test_a_refused_host_call_changes_nothing(calls, alone):
    """tmax given to the radiance query is refused before anything is staged; the calls after it give what they give alone, on a
    buffer that an earlier call has filled."""
    r = _fresh()
    try:
        byName = dict(calls[1])
        first = "query_closest 257"
        assert np.array_equal(_words(byName[first](r)), alone[first])
        o = np.zeros((65, 3), np.float32)
        d = np.tile(np.array((0, 0, 1), np.float32), (65, 1))
        t = np.ones(65, np.float32)
        out = np.zeros((65, 4), np.float32)
        batch = _capi.RtRayBatch(o.ctypes.data, d.ctypes.data, t.ctypes.data, 65)
        p = _capi.RtRadianceParams(1, 8, 1, 0)
        with pytest.raises(engine.RtError, match="tmax must be NULL"):
            r._check(r._l.rt_query_radiance_host(r._h, C.byref(batch), None, C.byref(p), None, out.ctypes.data), "rt_query_radiance_host")
        assert not out.any(), "a refused call writes nothing"
        for name in ("query_radiance 65 ids progressive", "query_occluded 65"):
            assert np.array_equal(_words(byName[name](r)), alone[name]), f"{name} after a refused call"
    finally:
        r.close()
