"""The render path's state of an instance (mi_pt_api.hip: the frame queue, the ring of frame constants, the sky constants, the second stream
of the shadow stage, the launch timer, and the order of operations of mi_pt_render_frames), characterised: scripted sequences of calls over
two tiny scenes, and after EVERY call one record -- the call's outcome (code and mi_pt_last_error when refused) and the three totals of
mi_pt_get_memory.  A step that reads adds the SHA-1 of what it read (accumulator, depth, selection, a denoised or a motion image), the
path-level counters (cameraPaths, segments, shadowRays, surfaceHits, textureTaps) and, with the launch timer on, the six integer launch
counters of mi_pt_get_frame_timing.  Only reading steps carry counters: mi_pt_get_stats and mi_pt_get_frame_timing issue the frames a queue
holds back and synchronise, which is exactly what the queue and ring sequences must not do between their calls.  The walks' node and
triangle counts and the timer's millisecond fields are left out: they vary with the dynamic feed and the clock.

The journal is compared record by record with tests/golden/render_state_journal.json, written by the library as it stood before the
render path's state had owners of its own: a change to that code that changes what an instance reports at any step shows up here.

One sequence per rule of that code: A the three ways to issue five frames (one by one, a batch, a queue with a read, re-sent and changed
frame constants and a parameter change in the middle, on a stream of the caller's); B more unsynchronised calls than the ring of frame
constants has slots; C growth of the path arrays, 64 frames being the pixel-major slot layout; D multi-sample frames, the guides and the
second moment they feed (shown by mi_pt_denoise_svgf); E a shadow-catcher frame (state by slot, the longer loop) and a plain one after it;
F the shadow stage on a second stream against one stream, and a bounce loop cut short (the survivor flush); G the other primary stages --
BVH2 walk, MI_PT_NO_PACKET, bound camera rays, a debug view; H the work after a first-frame batch with motion vectors on; I the
MI_PT_TRACE_SPANS diagnostics in a child process (its stderr lines, frame / it / rays, are in the journal); J every refusal of the render
calls, directly and through the queue, each followed by a render that must give the unrefused image.

Two journals written by the same library were equal in every field.

`python tests/test_gpu_render_state.py OUT.json` (the repository root on PYTHONPATH) writes the journal of the library in use."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_state_journal.json")
BOX = os.path.join(ROOT, "assets", "Box.glb")
W, H, TILE = 40, 24, 16   # the box: 3 x 2 tiles, the last column and row partly outside the image
GW, GH, GDEPTH = 32, 20, 4  # the glass scene (volume scatter: the polled, long bounce loop)
COUNTERS = ("cameraPaths", "segments", "shadowRays", "surfaceHits", "textureTaps")
MEMORY = ("sceneBytes", "rendererBytes", "pathStateBytes")
LAUNCHES = ("traceClosestLaunches", "shadeLaunches", "traceShadowLaunches", "bounceIterations", "tracePrimaryLaunches", "shadeFirstLaunches")
GUIDES = capi.MI_PT_USE_OPTIX_DENOISER
SPAN_LINE = re.compile(r"\[mi_pt span\] frame (\d+) it +(\d+) rays +(\d+) ")


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


class _Rig:
    """One instance, the frame constants it renders with, and the journal of its calls."""

    def __init__(self, journal, scene, width=W, height=H, max_depth=5, env=None, timing=False, ready=True, **kw):
        self.journal, self.tr, self.timing, self.size = journal, None, False, (width, height)
        self.fi, pixel_angle, focal = ptmod.camera_frame_info(scene.camera(0), width, height)
        self.sky = ptmod.default_sky()
        self.params = ptmod.default_params()
        self.params.maxDepth, self.params.numSamples, self.params.pixelAngle, self.params.focalDistance = max_depth, 1, pixel_angle, focal

        def create():  # (run-time switches are read once, at mi_pt_create)
            os.environ.update(env or {})
            try:
                self.tr = ptmod.PathTracer(scene, collect_counters=True, **kw)
            finally:
                for k in env or {}:
                    del os.environ[k]
        self.call("create", create)
        self.call("set_tile_partition", lambda: self.tr.set_tile_partition(0, 1, TILE))
        if ready:
            self.ready()
        if timing:
            self.call("enable_timing", lambda: self.tr.enable_timing(True))
            self.timing = True

    def ready(self):
        self.call("resize", lambda: self.tr.resize(*self.size))
        self.call("set_frame_info", lambda: self.tr.set_frame_info(self.fi))
        self.call("set_sky", lambda: self.tr.set_sky(self.sky))

    def call(self, step, fn, reads=False):
        record = {"step": step, "outcome": "ok"}
        try:
            got = fn()
            if reads:
                record.update(got)
        except ptmod.MiError as e:
            rc, message = re.match(r"libmi_pt: rc=(-?\d+): (.*)", str(e), re.S).groups()
            record["outcome"] = {"rc": int(rc), "message": message}
        if self.tr is not None:
            m = self.tr.memory()
            record["memory"] = {k: m[k] for k in MEMORY}
        self.journal.append(record)
        return record

    def p(self, frame, total, first=None, **fields):
        """The parameters of frame `frame` after `total` samples; a first frame (it overwrites the accumulator) when total is 0."""
        q = capi.MiPathtraceParams()
        C.memmove(C.byref(q), C.byref(self.params), C.sizeof(q))
        q.frameCount, q.totalSamples = frame, total
        if total == 0 if first is None else first:
            q.flags |= capi.MI_PT_FIRST_FRAME
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    def frame(self, params, stream=None, step=None):
        return self.call(step or "render_frame(%d)" % params.frameCount, lambda: self.tr.render_frame(params, stream))

    def frames(self, params, n, stream=None, step=None):
        return self.call(step or "render_frames(%d, %d)" % (params.frameCount, n), lambda: self.tr.render_frames(params, n, stream))

    def read(self, step="read", images=("accum", "depth", "selection")):
        def fn():
            got = {k: _sha(getattr(self.tr, "read_" + k)()) for k in images}
            s = self.tr.stats()
            got["stats"] = {k: s[k] for k in COUNTERS}
            if self.timing:
                t = self.tr.frame_timing()
                got["launches"] = {k: int(t[k]) for k in LAUNCHES}
            return got
        return self.call(step, fn, reads=True)

    def svgf(self, step):
        return self.call(step, lambda: {"svgf": _sha(self.tr.denoise_svgf(iterations=2))}, reads=True)

    def close(self):
        if self.tr is not None:
            self.tr.close()


class _Stream:
    """A stream of the caller's, made by the HIP runtime libmi_pt.so itself is linked to: the runtime's symbols are looked up through the
    library's handle, which searches its dependencies -- a process that has loaded torch as well holds a second runtime, which is not it."""

    def __init__(self):
        self.hip = capi.pt_lib()
        self.hip.hipStreamCreate.argtypes, self.hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p]
        s = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(s)) == 0 and s.value
        self.handle = s.value

    def close(self):
        assert self.hip.hipStreamDestroy(self.handle) == 0


IMAGES = ("accum", "depth", "selection")


def _same(a, b, fields=IMAGES):
    assert {k: a[k] for k in fields} == {k: b[k] for k in fields}, (a, b)


def _batching(box, glass, j):
    one = _Rig(j, box, timing=True)
    for f in range(5):
        one.frame(one.p(f, f))
    by_one = one.read()
    one.close()
    batch = _Rig(j, box, timing=True)
    batch.frames(batch.p(0, 0), 5)
    as_batch = batch.read()
    batch.close()
    _same(by_one, as_batch, fields=IMAGES + ("stats",))
    assert as_batch["launches"]["shadeLaunches"] * 5 == by_one["launches"]["shadeLaunches"], (by_one, as_batch)
    q, stream = _Rig(j, box, timing=True), _Stream()
    q.call("set_frame_queue(4)", lambda: q.tr.set_frame_queue(4))
    q.frame(q.p(0, 0), stream.handle)
    q.frame(q.p(1, 1), stream.handle)
    q.read("a read in the middle: a batch of 2", images=("accum",))
    q.frame(q.p(2, 2), stream.handle)
    q.call("the same frame info again: no flush", lambda: q.tr.set_frame_info(q.fi))
    q.call("the same sky again: no flush", lambda: q.tr.set_sky(q.sky))
    q.frame(q.p(3, 3), stream.handle)
    q.frame(q.p(4, 4), stream.handle)
    queued = q.read("a read: a batch of 3")
    _same(by_one, queued, fields=IMAGES + ("stats",))
    assert queued["launches"]["shadeLaunches"] == 2 * as_batch["launches"]["shadeLaunches"], (queued, as_batch)  # (two batches: the re-sent constants issued none)
    q.frame(q.p(5, 5), stream.handle)
    q.frame(q.p(6, 6, maxDepth=3), stream.handle, step="render_frame(6), maxDepth 3: flushes frame 5, starts a batch")
    q.frame(q.p(7, 7, maxDepth=3), stream.handle)
    q.sky.haze = 0.4
    q.call("a changed sky: flushes, and the sky constants are computed again", lambda: q.tr.set_sky(q.sky))
    q.frame(q.p(8, 8, maxDepth=3), stream.handle)
    q.frame(q.p(9, 9, maxDepth=3), None, step="render_frame(9) on the null stream: flushes frame 8, starts a batch")
    q.read("a read: batches of 1, 2, 1 and 1")
    q.close()
    stream.close()


def _ring_wrap(box, glass, j):
    r = _Rig(j, box)
    for f in range(40):  # (the ring has 32 slots: call 33 waits for the batch of call 1)
        r.frame(r.p(f, f))
    r.read()
    r.close()


def _growth(box, glass, j):
    r, done = _Rig(j, box), 0
    for n in (1, 3, 64, 2):
        r.frames(r.p(done, done), n)
        done += n
        r.read("read after %d frames" % done)
    r.close()


def _optional_arrays(box, glass, j):
    r, done = _Rig(j, box), 0
    for step, flags in (("two samples, guides on", GUIDES), ("guides off", 0), ("guides on again", GUIDES)):
        n = 2 if done == 0 else 1
        r.frames(r.p(done // 2, done, numSamples=2, flags=flags | (capi.MI_PT_FIRST_FRAME if done == 0 else 0)), n, step=step)
        done += 2 * n
        r.read("read: " + step)
        r.svgf("denoise_svgf: " + step)
    r.close()
    # ... and an accumulation that carries the guides throughout: the second moment covers it
    r = _Rig(j, box)
    for f in range(5):
        r.frame(r.p(f, f, flags=GUIDES | (capi.MI_PT_FIRST_FRAME if f == 0 else 0)))
    r.svgf("denoise_svgf: five frames with the guides")
    r.close()


def _catcher(box, glass, j):
    r = _Rig(j, box)
    plain_flags = r.fi.flags
    r.fi.flags |= capi.MI_SCENE_USE_INFINITE_PLANE | capi.MI_SCENE_INFINITE_PLANE_SHADOW_CATCHER
    r.fi.infinitePlaneDistance = -0.6
    r.call("set_frame_info: shadow catcher", lambda: r.tr.set_frame_info(r.fi))
    r.frames(r.p(0, 0), 2)
    r.read("read: catcher")
    r.fi.flags = plain_flags
    r.call("set_frame_info: plain", lambda: r.tr.set_frame_info(r.fi))
    r.frames(r.p(0, 0), 2)
    plain = r.read("read: plain after catcher")
    r.close()
    r = _Rig(j, box)
    r.frames(r.p(0, 0), 2)
    _same(plain, r.read("read: plain on a fresh instance"))
    r.close()


def _second_stream(box, glass, j):
    got = {}
    for name, env in (("two streams", {"MI_PT_OVERLAP_MIN_TRIS": "0"}), ("one stream", {"MI_PT_OVERLAP": "0"})):
        r = _Rig(j, box, env=env, timing=True)
        r.frame(r.p(0, 0))
        r.frames(r.p(1, 1), 2)
        r.frames(r.p(3, 3, numSamples=2), 1)
        got[name] = r.read("read: " + name)
        r.close()
    _same(got["two streams"], got["one stream"], fields=IMAGES + ("stats", "launches"))
    for name, env in (("whole loops", {}), ("loops cut after 2 iterations", {"MI_PT_DIAG_MAX_ITERS": "2"})):
        r = _Rig(j, glass, GW, GH, GDEPTH, env=env, timing=True)
        r.frame(r.p(0, 0))
        r.frames(r.p(1, 1), 2)
        got[name] = r.read("read: " + name)
        r.close()
    assert got["loops cut after 2 iterations"]["launches"]["bounceIterations"] == 4 < got["whole loops"]["launches"]["bounceIterations"], got


def _primary_stages(box, glass, j):
    got = {}
    for name, env, kw in (("packet walk", {}, {}), ("BVH2 walk", {}, {"bvh": 1}), ("MI_PT_NO_PACKET", {"MI_PT_NO_PACKET": "1"}, {})):
        r = _Rig(j, box, env=env, timing=True, **kw)
        r.frames(r.p(0, 0), 2)
        got[name] = r.read("read: " + name)
        if name == "packet walk":  # the same two frames again, from the built-in camera's own rays
            rays = r.tr.make_camera_rays(r.p(0, 0), 2)
            r.call("set_camera_rays", lambda: r.tr.set_camera_rays(rays, unit=True))
            r.frames(r.p(0, 0), 2)
            got["bound rays"] = r.read("read: bound camera rays")
            r.call("unbind", lambda: r.tr.set_camera_rays(None))
            r.fi.visualization = int(capi.Visualization.NORMAL_SHADING)
            r.call("set_frame_info: a debug view", lambda: r.tr.set_frame_info(r.fi))
            r.frames(r.p(0, 0), 2)
            r.read("read: debug view")
        r.close()
    for name in ("BVH2 walk", "MI_PT_NO_PACKET"):
        _same(got["packet walk"], got[name])
    # (the selection image follows the bound set's sample rays, not the built-in camera's own selection rays: journalled, not compared here)
    _same(got["packet walk"], got["bound rays"], fields=("accum", "depth"))
    assert got["packet walk"]["launches"]["tracePrimaryLaunches"] == 1 and got["MI_PT_NO_PACKET"]["launches"]["tracePrimaryLaunches"] == 0, got


def _first_frame(box, glass, j):
    r = _Rig(j, box)
    r.call("set_temporal", lambda: r.tr.set_temporal(True))
    r.frames(r.p(0, 0), 2)
    r.read("read: first-frame batch")
    r.call("read_motion", lambda: {"motion": _sha(r.tr.read_motion()), "firstHit": _sha(r.tr.read_first_hit())}, reads=True)
    r.frames(r.p(2, 2), 2)
    r.call("read_motion after a batch that is no first frame", lambda: {"motion": _sha(r.tr.read_motion())}, reads=True)
    r.close()


def _spans_run(journal, box, env):
    r = _Rig(journal, box, env=env, timing=True)
    r.frame(r.p(0, 0))
    r.frames(r.p(1, 1), 2)
    got = r.read()
    r.close()
    return got


def _trace_spans(box, glass, j):
    plain = _spans_run(j, box, {})
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-spans-child"], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")])))
    assert child.returncode == 0, (child.stdout[-2000:], child.stderr[-2000:])
    got = json.loads(child.stdout.strip().splitlines()[-1])
    _same(plain, got)
    lines = [line for line in child.stderr.splitlines() if line.startswith("[mi_pt span]")]
    spans = [[int(v) for v in SPAN_LINE.match(line).groups()] for line in lines]
    assert len(spans) == got["launches"]["bounceIterations"] > 0, (spans, got)
    j.append({"step": "MI_PT_TRACE_SPANS=1 in a child process", "read": got, "spans [frame, it, rays]": spans})


def _refusals(box, glass, j):
    base = _Rig(j, box)
    base.frame(base.p(0, 0))
    unrefused = base.read("read: the unrefused frame")
    base.close()
    for queue in (1, 4):
        r = _Rig(j, box, ready=False)
        if queue > 1:
            r.call("set_frame_queue(%d)" % queue, lambda: r.tr.set_frame_queue(queue))

        def refused(step, fn):
            """`fn` is refused by the call itself, then frame 0 renders as ever"""
            assert r.call(step, fn)["outcome"] != "ok", j[-1]
            if r.tr.width:
                r.frame(r.p(0, 0))
                _same(unrefused, r.read("read after: " + step))
        refused("render before resize", lambda: r.tr.render_frame(r.p(0, 0)))
        r.ready()
        refused("numSamples 0", lambda: r.tr.render_frame(r.p(0, 0, numSamples=0)))
        refused("maxDepth 0", lambda: r.tr.render_frame(r.p(0, 0, maxDepth=0)))
        refused("maxDepth 256", lambda: r.tr.render_frame(r.p(0, 0, maxDepth=256)))
        refused("numFrames 0", lambda: r.tr.render_frames(r.p(0, 0), 0))
        refused("numFrames 1025", lambda: r.tr.render_frames(r.p(0, 0), 1025))
        plain_flags = r.fi.flags
        r.fi.flags |= capi.MI_SCENE_USE_HDR_ENVIRONMENT
        r.call("set_frame_info: HDR flag", lambda: r.tr.set_frame_info(r.fi))
        # (held back by the queue, this one is reported by the call that issues the frame: mi_pt_render_frame's own checks do not cover it)
        hdr = r.call("HDR flag with no environment", lambda: r.tr.render_frame(r.p(0, 0)))
        if queue > 1 and hdr["outcome"] == "ok":
            hdr = r.call("HDR flag with no environment: synchronize", lambda: r.tr.synchronize())
        assert hdr["outcome"] != "ok", hdr
        r.fi.flags = plain_flags
        r.call("set_frame_info: plain", lambda: r.tr.set_frame_info(r.fi))
        r.frame(r.p(0, 0))
        _same(unrefused, r.read("read after: HDR flag with no environment"))
        rays = r.tr.make_camera_rays(r.p(0, 0), 1)
        r.call("set_camera_rays", lambda: r.tr.set_camera_rays(rays, unit=True))
        r.call("resize to another size", lambda: r.tr.resize(W + 8, H))
        r.call("rays bound at another size", lambda: r.tr.render_frame(r.p(0, 0)))
        assert j[-1]["outcome"] != "ok", j[-1]
        r.call("unbind", lambda: r.tr.set_camera_rays(None))
        r.call("resize back", lambda: r.tr.resize(W, H))
        r.frame(r.p(0, 0))
        _same(unrefused, r.read("read after: rays bound at another size"))
        r.close()


SEQUENCES = {"A batching": _batching, "B ring wrap": _ring_wrap, "C growth": _growth, "D optional arrays and moments": _optional_arrays,
             "E catcher": _catcher, "F second stream and truncated loops": _second_stream, "G other primary stages": _primary_stages,
             "H first-frame work": _first_frame, "I trace spans": _trace_spans, "J refusals": _refusals}


def _scenes(tmp):
    return ptmod.Scene(BOX), ptmod.Scene(scenegen.scene_glass_class(os.path.join(str(tmp), "glass.glb"), seed=9, tess=16))


def _journal(tmp, name):
    records = []
    SEQUENCES[name](*_scenes(tmp), records)
    return json.loads(json.dumps(records))  # (as the golden file holds it)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_these_sequences(golden):
    assert sorted(golden) == sorted(SEQUENCES)


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_journal_equals_the_one_recorded_before_the_render_state_had_owners(name, golden, tmp_path):
    got, want = _journal(tmp_path, name), golden[name]
    for k, (g, w) in enumerate(zip(got, want)):
        print(name, k, json.dumps(g))
        assert g == w, (name, k, g["step"], {f: (g.get(f), w.get(f)) for f in set(g) | set(w) if g.get(f) != w.get(f)})
    assert len(got) == len(want), (name, len(got), len(want))


if __name__ == "__main__":
    if sys.argv[1] == "--trace-spans-child":  # sequence I: the same frames under the synchronising diagnostics; the span lines go to stderr
        print(json.dumps(_spans_run([], ptmod.Scene(BOX), {"MI_PT_TRACE_SPANS": "1"})))
        sys.exit(0)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = {name: _journal(tmp, name) for name in sorted(SEQUENCES)}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
