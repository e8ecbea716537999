"""Thin Python handles over the C-ABI (include/mi_pt.h, include/mi_host.h) for tests, bench.py and tooling.

Mirrors the reference's host objects for the path-trace mode only:
  Scene            ~ nvvkgltf::Scene::load + SceneVk tables          (src/gltf_scene.cpp:298, src/gltf_scene_vk.cpp:218)
  HdrEnvironment   ~ nvvk::HdrIbl::loadEnvironment                   (src/renderer.cpp:1982-2017)
  PathTracer       ~ class PathTracer : BaseRenderer                 (src/renderer_pathtracer.cpp:500-614)
  HeadlessRenderer ~ the GltfRenderer::onRender slice that drives it (src/renderer.cpp:588-742, :1959-1977)
Everything numerical happens inside libmi_pt.so (HIP); there is no Python or CPU fallback for rendering.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


# MiPtRayHit (include/mi_pt.h) as a structured numpy record: 64 bytes
HIT_DTYPE = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("flags", "<u4"), ("renderNode", "<i4"), ("renderPrimID", "<i4"), ("triangle", "<u4"),
                      ("materialID", "<i4"), ("position", "<f4", (3,)), ("reserved0", "<f4"), ("normal", "<f4", (3,)), ("reserved1", "<f4")])
assert HIT_DTYPE.itemsize == 64
_QUERY_MODES = {"closest": capi.MI_PT_QUERY_CLOSEST, "any": capi.MI_PT_QUERY_ANY, "nearest_k": capi.MI_PT_QUERY_NEAREST_K}
_QUERY_ALPHA = {"opaque": capi.MI_PT_QUERY_ALPHA_OPAQUE, "cutoff": capi.MI_PT_QUERY_ALPHA_CUTOFF, "stochastic": capi.MI_PT_QUERY_ALPHA_STOCHASTIC}
_QUERY_CULL = {"none": capi.MI_PT_QUERY_CULL_NONE, "material": capi.MI_PT_QUERY_CULL_MATERIAL}


class MiError(RuntimeError):
    pass


def _check_host(rc):
    if rc != 0:
        raise MiError(f"libmi_host: rc={rc}: {capi.host_lib().mi_host_last_error().decode()}")


def _check_pt(rc):
    if rc != 0:
        raise MiError(f"libmi_pt: rc={rc}: {capi.pt_lib().mi_pt_last_error().decode()}")


class Scene:
    def __init__(self, path):
        self._h = capi.host_lib()
        self._p = C.c_void_p()
        _check_host(self._h.mi_scene_load(str(path).encode(), C.byref(self._p)))
        self.path = str(path)

    @property
    def desc(self):
        return self._h.mi_scene_desc(self._p)

    @property
    def num_triangles(self):
        return int(self._h.mi_scene_num_triangles(self._p))

    @property
    def num_cameras(self):
        return int(self._h.mi_scene_num_cameras(self._p))

    def camera(self, index=0):
        cam = capi.MiCamera()
        _check_host(self._h.mi_scene_camera(self._p, index, C.byref(cam)))
        return cam

    def recompute_tangents(self, force_creation=True, mikktspace=True):
        """recomputeTangents of the reference (src/gltf_create_tangent.hpp:40); returns the vertices added by the MikkTSpace splitting.
        The scene's desc changes: create PathTracers after this call."""
        n = self._h.mi_scene_recompute_tangents(self._p, int(force_creation), int(mikktspace))
        if n < 0:
            _check_host(n)
        return n

    def cut_alpha(self, subdivisions=8):
        """Load-time bake for alpha-MASK geometry (mi_scene_cut_alpha): drops the parts of alpha-tested triangles on which the test
        cannot pass.  Returns the number of (sub-)triangles dropped.  The scene's desc changes: create PathTracers after this call."""
        n = self._h.mi_scene_cut_alpha(self._p, int(subdivisions))
        if n < 0:
            _check_host(int(n))
        return int(n)

    @property
    def variants(self):
        """The names of the KHR_materials_variants of the file, in order ([] without the extension)."""
        out = []
        for i in range(int(self._h.mi_scene_num_variants(self._p))):
            name = C.create_string_buffer(256)
            _check_host(self._h.mi_scene_variant_name(self._p, i, name, 256))
            out.append(name.value.decode())
        return out

    @property
    def current_variant(self):
        return int(self._h.mi_scene_current_variant(self._p))

    def set_variant(self, variant):
        """Switches the material variant (mi_scene_set_variant): the material ids of the render-node table of `desc` change in place.  Returns
        the number of render nodes whose material changed; follow with PathTracer.update_render_nodes (a patch in resident mode, a
        rebuild otherwise).  Raises MiError, with nothing changed, for a variant out of range or an alpha change on cut geometry."""
        n = self._h.mi_scene_set_variant(self._p, int(variant))
        if n < 0:
            _check_host(n)
        return int(n)

    @property
    def num_animations(self):
        return int(self._h.mi_scene_num_animations(self._p))

    def animation_info(self, index=0):
        """(name, start, end) of a clip (AnimationInfo of the reference, src/gltf_scene.hpp:159-189)."""
        a, b, name = C.c_float(), C.c_float(), C.create_string_buffer(256)
        _check_host(self._h.mi_scene_animation_info(self._p, index, C.byref(a), C.byref(b), name, 256))
        return name.value.decode(), a.value, b.value

    def update_animation(self, index, time):
        """Poses the scene at `time`: the render-node matrices and light placements of `desc` change in place -- and, for
        KHR_animation_pointer channels, its material, texture-info and light tables, visibility flags and cameras.  True when something
        moved; follow with PathTracer.update_from_scene(scene).  animation_changes says what changed."""
        r = self._h.mi_scene_update_animation(self._p, index, float(time))
        if r < 0:
            _check_host(r)
        return bool(r)

    @property
    def animation_changes(self):
        """capi.MI_SCENE_CHANGED_* bits of the last update_animation (mi_scene_animation_changes)."""
        return int(self._h.mi_scene_animation_changes(self._p))

    @property
    def deformation(self):
        """The skin / morph tables (capi.MiPtDeformDesc, mi_scene_deformation) or None when the scene deforms nothing.  Its frame arrays
        (joint matrices, morph weights) follow every update_animation in place."""
        d = self._h.mi_scene_deformation(self._p)
        return d.contents if d else None

    def deform_on_host(self):
        """Writes the posed vertices of the current frame into the scene's own render-primitive streams (the CPU restatement of the
        device kernel), so that a PathTracer created afterwards, or the oracle, sees the pose.  Returns the primitives deformed."""
        n = self._h.mi_scene_deform_on_host(self._p)
        if n < 0:
            _check_host(n)
        return n

    def bounds(self):
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        self._h.mi_scene_bounds(self._p, lo, hi)
        return np.array(lo[:]), np.array(hi[:])

    def close(self):
        if self._p:
            self._h.mi_scene_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HdrEnvironment:
    def __init__(self, path=None, pixels=None):
        self._h = capi.host_lib()
        self._p = C.c_void_p()
        if path is not None:
            _check_host(self._h.mi_hdr_load(str(path).encode(), C.byref(self._p)))
        else:
            px = np.ascontiguousarray(pixels, dtype=np.float32)
            assert px.ndim == 3 and px.shape[2] == 3
            _check_host(self._h.mi_hdr_from_pixels(px.shape[1], px.shape[0], px.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._p)))

    @property
    def env(self):
        return self._h.mi_hdr_env(self._p)

    def close(self):
        if self._p:
            self._h.mi_hdr_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_sky():
    sky = capi.MiSkyPhysicalParameters()
    capi.host_lib().mi_default_sky(C.byref(sky))
    return sky


def default_params():
    p = capi.MiPathtraceParams()
    capi.host_lib().mi_default_params(C.byref(p))
    return p


def camera_frame_info(cam, width, height, visualization=0):
    """Returns (MiSceneFrameInfo, pixelAngle, focalDistance) — reference: src/renderer.cpp:675-705.  visualization: a debug view
    (capi.Visualization); 0 is the path-traced image."""
    fi, pa, fd = capi.MiSceneFrameInfo(), C.c_float(), C.c_float()
    capi.host_lib().mi_camera_frame_info(C.byref(cam), width, height, C.byref(fi), C.byref(pa), C.byref(fd))
    fi.visualization = int(visualization)
    return fi, pa.value, fd.value


_PROJECTIONS = {"perspective": capi.MI_PROJECTION_PERSPECTIVE, "equirect": capi.MI_PROJECTION_EQUIRECT, "fisheye": capi.MI_PROJECTION_FISHEYE}


def camera_rays(cam, width, height, projection="equirect", fov=180.0, jitter=None):
    """Camera rays of the pose of `cam` under a projection (mi_camera_rays, include/mi_host.h): "perspective" (the built-in camera without its
    lens), "equirect" (a 360 degree panorama) or "fisheye" (equidistant, `fov` degrees across the image circle; outside it the rays are dead).
    jitter: None (pixel centres, one set) or (K, 2) sample offsets inside the pixel, one set per row.  Returns (rays, pixel_angle): a
    (K, height, width, 8) float32 array for PathTracer.set_camera_rays -- unit directions -- and the params.pixelAngle of the projection."""
    proj = _PROJECTIONS[projection] if isinstance(projection, str) else int(projection)
    jit = None if jitter is None else np.ascontiguousarray(jitter, dtype=np.float32).reshape(-1, 2)
    k = 1 if jit is None else int(jit.shape[0])
    rays = np.zeros((k, int(height), int(width), 8), dtype=np.float32)
    pa = C.c_float()
    _check_host(capi.host_lib().mi_camera_rays(C.byref(cam), proj, float(fov), int(width), int(height),
                                               None if jit is None else jit.ctypes.data_as(C.POINTER(C.c_float)), k,
                                               rays.ctypes.data_as(C.POINTER(capi.MiPtRay)), C.byref(pa)))
    return rays, pa.value


class PathTracer:
    """The HIP path tracer instance (libmi_pt.so)."""

    def __init__(self, scene, device=0, collect_counters=False, bvh=0):
        """bvh: MiPtCreateOptions::bvhBuilder, two bits.  Bit 0: the walk -- 0 the 8-wide compressed BVH (default), 1 the plain BVH2.  Bit 1: the
        topology of the BVH2 both are made from -- 0 PLOC clustering over the Morton order (default), 2 the Karras Morton-prefix hierarchy.  So 0 .. 3;
        the images and the query records do not depend on it."""
        self._l = capi.pt_lib()
        self._p = C.c_void_p()
        self._scene = scene  # keep host tables alive for the duration of mi_pt_create only (they are copied)
        opts = capi.MiPtCreateOptions()
        opts.device = device
        opts.collectCounters = 1 if collect_counters else 0
        opts.bvhBuilder = bvh  # bit 0: 0 = 8-wide compressed BVH (default), 1 = plain BVH2; bit 1: 0 = PLOC clustering (default), 1 (bvh = 2, 3) = Karras topology
        _check_pt(self._l.mi_pt_create(scene.desc, C.byref(opts), C.byref(self._p)))
        self.width = self.height = 0
        self.temporal = False
        self._camera_rays = None  # the device tensor set_camera_rays borrowed
        self._device = int(device)

    def update_render_nodes(self, render_nodes, count, visible=None):
        """New transforms / materials / visibility for the instances: rebuilds the acceleration structure on the device (or refits and
        patches it: set_accel_update, set_accel_resident)."""
        _check_pt(self._l.mi_pt_update_render_nodes(self._p, render_nodes, count, visible))

    def update_lights(self, lights, count):
        """New placement / colour / cone of the lights (same count as at creation)."""
        _check_pt(self._l.mi_pt_update_lights(self._p, lights, count))

    def update_materials(self, materials, num_materials, texture_infos, num_texture_infos):
        """New material and texture-info tables (mi_pt_update_materials): the same number of materials as at creation; everything a build
        derives from them is updated in place, with a rebuild only where include/mi_pt.h lists one.  Restart the accumulation afterwards."""
        _check_pt(self._l.mi_pt_update_materials(self._p, materials, int(num_materials), texture_infos, int(num_texture_infos)))

    def set_deformation(self, scene):
        """Static upload of the scene's skin / morph tables (mi_pt_set_deformation); None, or a scene without deformers, releases them."""
        d = scene.deformation if scene is not None else None
        _check_pt(self._l.mi_pt_set_deformation(self._p, C.byref(d) if d is not None else None))
        self._deforming = d is not None

    def update_deformation(self, joint_matrices, morph_weights, defer_build=False):
        """Deforms every skinned / morphed primitive on the device from this frame's packed tables (ctypes float pointers or float32 arrays),
        then rebuilds the acceleration structure unless defer_build (the caller calls update_render_nodes next)."""
        def keep(a):  # a float32 array that lives across the call, or the ctypes pointer as given
            return a if a is None or isinstance(a, C._Pointer) else np.ascontiguousarray(a, dtype=np.float32)

        def ptr(a):
            return a if a is None or isinstance(a, C._Pointer) else a.ctypes.data_as(C.POINTER(C.c_float))
        jm, mw = keep(joint_matrices), keep(morph_weights)
        _check_pt(self._l.mi_pt_update_deformation(self._p, ptr(jm), ptr(mw), capi.MI_PT_DEFORM_DEFER_BUILD if defer_build else 0))

    def set_vertex_updates(self, prims, recompute_normals=False):
        """Declares the render primitives whose vertices the caller drives (mi_pt_set_vertex_updates); None or an empty list releases the
        declaration.  recompute_normals: an update that brings no normals for a primitive with a normal stream rebuilds them on the device
        (area-weighted face normals; tangents are never rebuilt -- supply them where a normal map needs them)."""
        ids = [int(p) for p in (prims if prims is not None else [])]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        _check_pt(self._l.mi_pt_set_vertex_updates(self._p, arr, len(ids), capi.MI_PT_VERTICES_RECOMPUTE_NORMALS if recompute_normals else 0))

    def update_vertices(self, updates, defer_build=False):
        """New vertices for declared primitives (mi_pt_update_vertices / mi_pt_update_vertices_device): {prim: positions} or
        {prim: (positions, normals, tangents)} with None for a stream that keeps its values.  Float32 numpy arrays (anything np.asarray takes)
        go through the host form; contiguous float32 torch tensors on this instance's device through the device form, read where they lie.
        Mixing the two in one call is an error.  The acceleration structure follows unless defer_build (update_render_nodes comes next)."""
        def is_device(a):
            return hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")
        table = (capi.MiPtVertexUpdate * max(len(updates), 1))()
        keep, forms = [], set()
        for k, (prim, streams) in enumerate(updates.items()):
            streams = tuple(streams) if isinstance(streams, (tuple, list)) else (streams,)
            if not 1 <= len(streams) <= 3 or streams[0] is None:
                raise ValueError(f"update_vertices: primitive {prim}: positions, or (positions, normals, tangents)")
            streams = streams + (None,) * (3 - len(streams))
            u = table[k]
            u.renderPrimID = int(prim)
            for name, a, width in zip(("positions", "normals", "tangents"), streams, (3, 3, 4)):
                if a is None:
                    continue
                forms.add(is_device(a))
                if is_device(a):
                    if str(a.dtype) != "torch.float32" or not a.is_contiguous() or a.device.type != "cuda":
                        raise ValueError(f"update_vertices: primitive {prim}: {name} must be a contiguous float32 tensor on the device")
                    count, ptr = a.numel(), a.data_ptr()
                else:
                    a = np.ascontiguousarray(a, dtype=np.float32)
                    count, ptr = a.size, a.ctypes.data
                keep.append(a)
                if count % width:
                    raise ValueError(f"update_vertices: primitive {prim}: {name} holds {count} floats, no multiple of {width}")
                if name == "positions":
                    u.vertexCount = count // width
                elif count // width != u.vertexCount:
                    raise ValueError(f"update_vertices: primitive {prim}: {name} has {count // width} vertices, positions {u.vertexCount}")
                setattr(u, name, ptr)
        if len(forms) > 1:
            raise ValueError("update_vertices: numpy arrays and device tensors in one call")
        fn = self._l.mi_pt_update_vertices_device if True in forms else self._l.mi_pt_update_vertices
        _check_pt(fn(self._p, table, len(updates), capi.MI_PT_DEFORM_DEFER_BUILD if defer_build else 0))

    def vertex_update_info(self):
        """mi_pt_get_vertex_update_info as a dict: calls, verticesWritten (both in total), verticesRejected (last call), tableBytes."""
        a = capi.MiPtVertexUpdateInfo()
        _check_pt(self._l.mi_pt_get_vertex_update_info(self._p, C.byref(a)))
        return {n: int(getattr(a, n)) for n, _ in a._fields_}

    def update_textures(self, updates, generate_mips=True):
        """New images for resident textures (mi_pt_update_textures / mi_pt_update_textures_device): {texture index: image}.  An image is an
        H x W x 4 array of the resident size: numpy uint8 (RGBA8) or float32 (linear RGBA32F, quantised on the device) through the host form,
        contiguous torch uint8 / float32 tensors on this instance's device through the device form, read where they lie.  generate_mips:
        the image is level 0 and the device makes the chain the host loader would; without it the value is the list of ALL levels, uint8.
        Mixing numpy arrays and device tensors in one call is an error.  Restart the accumulation afterwards."""
        def is_device(a):
            return hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")
        table = (capi.MiPtTextureUpdate * max(len(updates), 1))()
        keep, forms = [], set()
        for k, (index, levels) in enumerate(updates.items()):
            levels = list(levels) if isinstance(levels, (tuple, list)) else [levels]
            if not levels or (generate_mips and len(levels) != 1):
                raise ValueError(f"update_textures: texture {index}: one image with generate_mips, the list of all levels without")
            ptrs = (C.c_void_p * len(levels))()
            kinds = set()
            for l, a in enumerate(levels):
                forms.add(is_device(a))
                if is_device(a):
                    if str(a.dtype) not in ("torch.uint8", "torch.float32") or not a.is_contiguous() or a.device.type != "cuda":
                        raise ValueError(f"update_textures: texture {index}: level {l} must be a contiguous uint8 or float32 tensor on the device")
                    kinds.add(str(a.dtype) == "torch.float32")
                    shape, ptrs[l] = tuple(a.shape), a.data_ptr()
                else:
                    a = np.asarray(a)
                    if a.dtype not in (np.uint8, np.float32):
                        raise ValueError(f"update_textures: texture {index}: level {l} must be uint8 or float32, not {a.dtype}")
                    a = np.ascontiguousarray(a)
                    kinds.add(a.dtype == np.float32)
                    shape, ptrs[l] = a.shape, a.ctypes.data
                keep.append(a)
                if len(shape) != 3 or shape[2] != 4:
                    raise ValueError(f"update_textures: texture {index}: level {l} has shape {shape}, not H x W x 4")
                if l == 0:
                    height, width = int(shape[0]), int(shape[1])
                elif (int(shape[0]), int(shape[1])) != (max(1, height >> l), max(1, width >> l)):
                    raise ValueError(f"update_textures: texture {index}: level {l} has shape {shape}")
            if len(kinds) > 1:
                raise ValueError(f"update_textures: texture {index}: uint8 and float32 levels")
            keep.append(ptrs)
            u = table[k]
            u.texture, u.width, u.height, u.numLevels = int(index), width, height, len(levels)
            u.format = capi.MI_PT_TEXELS_RGBA32F if True in kinds else capi.MI_PT_TEXELS_RGBA8
            u.flags = capi.MI_PT_TEXTURE_GENERATE_MIPS if generate_mips else 0
            u.levels = C.cast(ptrs, C.POINTER(C.c_void_p))
        if len(forms) > 1:
            raise ValueError("update_textures: numpy arrays and device tensors in one call")
        fn = self._l.mi_pt_update_textures_device if True in forms else self._l.mi_pt_update_textures
        _check_pt(fn(self._p, table, len(updates)))

    def read_texture(self, index, level=0):
        """The resident texels of one level of texture `index` (mi_pt_read_texture): H x W x 4 uint8."""
        d = self._scene.desc.contents
        known = 0 <= int(index) < int(d.numTextures) and 0 <= int(level) < 16  # (the library refuses what is not)
        h, w = (int(d.textures[int(index)].height), int(d.textures[int(index)].width)) if known else (1, 1)
        out = np.zeros((max(1, h >> int(level)) if known else 1, max(1, w >> int(level)) if known else 1, 4), np.uint8)
        _check_pt(self._l.mi_pt_read_texture(self._p, int(index), int(level), out.ctypes.data))
        return out

    def texture_update_info(self):
        """mi_pt_get_texture_update_info as a dict: calls, texelsWritten, levelsGenerated (all in total), launches (last call)."""
        a = capi.MiPtTextureUpdateInfo()
        _check_pt(self._l.mi_pt_get_texture_update_info(self._p, C.byref(a)))
        return {n: int(getattr(a, n)) for n, _ in a._fields_}

    def update_environment(self, pixels):
        """A new HDR environment from its texels alone (mi_pt_update_environment / mi_pt_update_environment_device): an H x W x 3 or H x W x 4
        lat-long image, row 0 at the +Y pole; the input alpha is ignored.  A numpy float32 array (anything np.asarray takes) goes through the
        host form, which refuses non-finite and negative components; a contiguous float32 torch tensor on this instance's device through the
        device form, read where it lies, with such components replaced by 0.  The pdf and the alias table are made on the device; a size equal
        to the resident one is written in place.  Restart the accumulation afterwards."""
        device = hasattr(pixels, "data_ptr") and hasattr(pixels, "is_contiguous")
        if device:
            if str(pixels.dtype) != "torch.float32" or not pixels.is_contiguous() or pixels.device.type != "cuda":
                raise ValueError("update_environment: the tensor must be a contiguous float32 tensor on the device")
            shape, ptr = tuple(pixels.shape), pixels.data_ptr()
        else:
            pixels = np.ascontiguousarray(pixels, dtype=np.float32)
            shape, ptr = pixels.shape, pixels.ctypes.data
        if len(shape) != 3 or shape[2] not in (3, 4) or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"update_environment: the image has shape {shape}, not H x W x 3 or H x W x 4")
        u = capi.MiPtEnvironmentUpdate()
        u.width, u.height, u.channels, u.pixels = int(shape[1]), int(shape[0]), int(shape[2]), ptr
        fn = self._l.mi_pt_update_environment_device if device else self._l.mi_pt_update_environment
        _check_pt(fn(self._p, C.byref(u)))

    def read_environment(self):
        """The resident environment (mi_pt_read_environment): (rgba, alias, q, integral) -- H x W x 4 float32 with the pdf in alpha, H x W uint32
        and float32 of the alias table, the integral.  MiError (rc=-4) when none is resident."""
        w, h, integral = C.c_int32(), C.c_int32(), C.c_float()
        _check_pt(self._l.mi_pt_read_environment(self._p, None, None, C.byref(w), C.byref(h), C.byref(integral)))
        rgba = np.empty((h.value, w.value, 4), np.float32)
        accel = np.empty((h.value, w.value), np.dtype([("alias", "<u4"), ("q", "<f4")]))
        _check_pt(self._l.mi_pt_read_environment(self._p, rgba.ctypes.data, accel.ctypes.data, None, None, None))
        return rgba, np.ascontiguousarray(accel["alias"]), np.ascontiguousarray(accel["q"]), float(integral.value)

    def environment_update_info(self):
        """mi_pt_get_environment_update_info as a dict: calls, texelsWritten (in total); texelsSanitised, launches, lightTexels, heavyTexels,
        integral (last call); scratchBytes."""
        a = capi.MiPtEnvironmentUpdateInfo()
        _check_pt(self._l.mi_pt_get_environment_update_info(self._p, C.byref(a)))
        return {n: (float(a.integral) if n == "integral" else int(getattr(a, n))) for n, _ in a._fields_ if n != "reserved"}

    ACCEL_MODES = {"rebuild": 0, "refit": 1, "auto": 2}

    def set_accel_update(self, mode, rebuild_cost_ratio=1.5):
        """How animated frames update the acceleration structure (mi_pt_set_accel_update): "rebuild" / 0 (default), "refit" / 1 (the 8-wide
        tree refitted in place) or "auto" / 2 (refit while its SAH cost stays within rebuild_cost_ratio x the cost after the last build)."""
        m = self.ACCEL_MODES[mode] if isinstance(mode, str) else int(mode)
        _check_pt(self._l.mi_pt_set_accel_update(self._p, m, C.c_float(rebuild_cost_ratio)))

    def accel_info(self):
        """mi_pt_get_accel_info as a dict: mode, lastUpdate, builds, refits, SAH cost at the last build and now, triangles moved, refit bytes."""
        a = capi.MiPtAccelInfo()
        _check_pt(self._l.mi_pt_get_accel_info(self._p, C.byref(a)))
        return {n: getattr(a, n) for n, _ in a._fields_ if n != "reserved"}

    def set_accel_resident(self, enable=True):
        """Resident mode (mi_pt_set_accel_resident): with refits allowed (set_accel_update "refit" / "auto"), hidden render nodes stay in
        the tree, so that a visibility change is a refit and a material-id change a patch instead of a build.  ~130 B per hidden triangle."""
        _check_pt(self._l.mi_pt_set_accel_resident(self._p, 1 if enable else 0))

    def accel_resident_info(self):
        """mi_pt_get_accel_resident_info as a dict: enabled, inForce, residentTriangles, hiddenTriangles, visibilityRefits, materialPatches."""
        a = capi.MiPtAccelResidentInfo()
        _check_pt(self._l.mi_pt_get_accel_resident_info(self._p, C.byref(a)))
        return {n: getattr(a, n) for n, _ in a._fields_}

    def read_vertices(self, prim):
        """The resident streams of render primitive `prim`: (positions (V, 3), normals (V, 3) or None, tangents (V, 4) or None)."""
        p = self._scene.desc.contents.renderPrimitives[prim]
        n = int(p.vertexCount)
        pos = np.zeros((n, 3), np.float32)
        nrm = np.zeros((n, 3), np.float32) if p.normals else None
        tan = np.zeros((n, 4), np.float32) if p.tangents else None
        f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
        _check_pt(self._l.mi_pt_read_vertices(self._p, int(prim), f(pos), f(nrm), f(tan)))
        return pos, nrm, tan

    def update_from_scene(self, scene):
        """After Scene.update_animation: hands the scene's render-node and light tables to the device again -- and, after set_deformation,
        deforms the skinned / morphed geometry first (with the rebuild left to update_render_nodes: one per frame); the material tables
        only when a KHR_animation_pointer channel changed them.  A changed camera is the caller's: scene.camera() -> set_frame_info."""
        d = scene.desc.contents
        deform = scene.deformation if getattr(self, "_deforming", False) else None
        if deform is not None:
            self.update_deformation(deform.jointMatrices, deform.morphWeights, defer_build=True)
        if scene.animation_changes & capi.MI_SCENE_CHANGED_MATERIALS:  # (KHR_animation_pointer; before the nodes: a rebuild then sees the new flags)
            self.update_materials(d.materials, d.numMaterials, d.textureInfos, d.numTextureInfos)
        self.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
        self.update_lights(d.lights, d.numLights)

    def set_environment(self, hdr):
        _check_pt(self._l.mi_pt_set_environment(self._p, hdr.env if hdr is not None else None))

    def resize(self, width, height):
        _check_pt(self._l.mi_pt_resize(self._p, width, height))
        self.width, self.height = width, height

    def set_frame_info(self, fi):
        _check_pt(self._l.mi_pt_set_frame_info(self._p, C.byref(fi)))

    def set_sky(self, sky):
        _check_pt(self._l.mi_pt_set_sky(self._p, C.byref(sky)))

    def set_tile_partition(self, rank, world, tile_size=64):
        _check_pt(self._l.mi_pt_set_tile_partition(self._p, rank, world, tile_size))

    def bind_accum(self, device_ptr):
        _check_pt(self._l.mi_pt_bind_accum(self._p, C.c_void_p(device_ptr)))

    def bind_guides(self, albedo_ptr=0, normal_ptr=0, depth_ptr=0):
        """Denoiser guide / depth images in caller-owned device memory (0 = the internal image)."""
        _check_pt(self._l.mi_pt_bind_guides(self._p, C.c_void_p(albedo_ptr or None), C.c_void_p(normal_ptr or None), C.c_void_p(depth_ptr or None)))

    def set_frame_queue(self, depth):
        """render_frame calls are held back and issued `depth` at a time as one batch (mi_pt_set_frame_queue); 1 = at once."""
        _check_pt(self._l.mi_pt_set_frame_queue(self._p, int(depth)))

    def render_frame(self, params, stream=None):
        _check_pt(self._l.mi_pt_render_frame(self._p, C.byref(params), C.c_void_p(stream or 0)))

    def render_frames(self, params, num_frames, stream=None):
        """num_frames frames in flight; bit-identical to num_frames successive render_frame calls (include/mi_pt.h)."""
        _check_pt(self._l.mi_pt_render_frames(self._p, C.byref(params), num_frames, C.c_void_p(stream or 0)))

    def synchronize(self):
        _check_pt(self._l.mi_pt_synchronize(self._p))

    def read_accum(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check_pt(self._l.mi_pt_read_accum(self._p, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def write_accum(self, img):
        img = np.ascontiguousarray(img, dtype=np.float32)
        assert img.shape == (self.height, self.width, 4)
        _check_pt(self._l.mi_pt_write_accum(self._p, img.ctypes.data_as(C.POINTER(C.c_float))))

    def read_guides(self):
        """(albedo RGBA, normal RGBA) guide layers of the denoiser (valid when MI_PT_USE_OPTIX_DENOISER was set)."""
        a = np.empty((self.height, self.width, 4), dtype=np.float32)
        n = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check_pt(self._l.mi_pt_read_guides(self._p, a.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_float))))
        return a, n

    def read_selection(self):
        out = np.empty((self.height, self.width), dtype=np.uint32)
        _check_pt(self._l.mi_pt_read_selection(self._p, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def set_camera_rays(self, rays, unit=False):
        """Start the following frames from the caller's rays instead of the built-in camera (mi_pt_set_camera_rays; include/mi_pt.h has the
        contract).  `rays`: (K, H, W, 8) or (H, W, 8) float32 rows of origin.xyz, tMin, direction.xyz, tMax at the current size -- frame F takes
        set F % K.  A numpy array is copied by the library; a contiguous torch tensor on this instance's device is borrowed (the wrapper keeps a
        reference; do not write to it while frames are in flight); None unbinds.  unit: the directions are unit vectors, used bit for bit."""
        flags = capi.MI_PT_CAMERA_RAYS_UNIT if unit else 0
        if rays is None:
            _check_pt(self._l.mi_pt_set_camera_rays(self._p, None, 0, 0))
            self._camera_rays = None
            return
        torch_form = type(rays).__module__.split(".")[0] == "torch"
        if not torch_form:
            rays = np.ascontiguousarray(rays, dtype=np.float32)
        shape = tuple(rays.shape)
        if len(shape) == 3:
            shape = (1,) + shape
        if len(shape) != 4 or shape[1:] != (self.height, self.width, 8) or shape[0] < 1:
            raise ValueError("set_camera_rays: a (K, %d, %d, 8) or (%d, %d, 8) float32 array is required" % (self.height, self.width, self.height, self.width))
        if torch_form:
            import torch
            if not (rays.is_cuda and rays.dtype == torch.float32 and rays.is_contiguous()):
                raise ValueError("set_camera_rays: a contiguous float32 device tensor is required")
            _check_pt(self._l.mi_pt_set_camera_rays_device(self._p, C.c_void_p(rays.data_ptr()), int(shape[0]), flags))
            self._camera_rays = rays
            return
        _check_pt(self._l.mi_pt_set_camera_rays(self._p, rays.ctypes.data_as(C.POINTER(capi.MiPtRay)), int(shape[0]), flags))
        self._camera_rays = None

    def make_camera_rays(self, params, num_sets=1, device=False, stream=None):
        """The rays the built-in camera generates for sample 0 of frames params.frameCount .. + num_sets - 1, for every pixel
        (mi_pt_make_camera_rays): (num_sets, H, W, 8) float32, numpy, or with device=True a torch tensor on this instance's device written on
        `stream` (default: torch's current stream).  Bound with unit=True they reproduce the built-in camera's single-sample frames."""
        if device:
            import torch
            out = torch.empty((int(num_sets), self.height, self.width, 8), dtype=torch.float32, device="cuda:%d" % self._device)
            if stream is None:
                stream = torch.cuda.current_stream(out.device).cuda_stream
            _check_pt(self._l.mi_pt_make_camera_rays_device(self._p, C.byref(params), int(num_sets), C.c_void_p(out.data_ptr()), C.c_void_p(stream or 0)))
            return out
        out = np.zeros((int(num_sets), self.height, self.width, 8), dtype=np.float32)
        _check_pt(self._l.mi_pt_make_camera_rays(self._p, C.byref(params), int(num_sets), out.ctypes.data_as(C.POINTER(capi.MiPtRay))))
        return out

    @staticmethod
    def _query_options(mode, alpha, cull, max_hits, blend_threshold, seed):
        """MiPtQueryOptions of the keyword arguments, or None when they are the defaults of the plain entry points (which then serve the call)."""
        m = _QUERY_MODES[mode] if isinstance(mode, str) else int(mode)
        a = _QUERY_ALPHA[alpha] if isinstance(alpha, str) else int(alpha)
        c = _QUERY_CULL[cull] if isinstance(cull, str) else int(cull)
        # (a call without any of the new arguments is the plain entry point's, whatever it passes for `mode`: "nearest_k" is one of the new arguments)
        if (mode != "nearest_k" and a == capi.MI_PT_QUERY_ALPHA_OPAQUE and c == capi.MI_PT_QUERY_CULL_NONE and int(max_hits) == 1
                and float(blend_threshold) == 0.5 and int(seed) == 0):
            return m, None
        o = capi.MiPtQueryOptions()
        o.mode, o.alpha, o.cull, o.maxHits, o.blendThreshold, o.seed = m, a, c, int(max_hits), float(blend_threshold), int(seed) & 0xffffffff
        return m, o

    def query_rays(self, rays, mode="closest", stream=None, alpha="opaque", cull="none", max_hits=1, blend_threshold=0.5, seed=0):
        """Rays against the resident scene (mi_pt_query_rays / mi_pt_query_rays_ex; include/mi_pt.h has the semantics).  `rays`: (n, 8) float32
        rows of origin.xyz, tMin, direction.xyz, tMax; mode "closest", "any" or "nearest_k" (the max_hits nearest distinct triangles per ray, 1..8);
        alpha "opaque" (every triangle counts), "cutoff" (opacity >= blend_threshold; MASK surfaces follow their own cutoff) or "stochastic" (the
        frames' draw, from `seed`); cull "none" or "material" (back faces of single-sided materials are skipped).  A numpy array returns a
        structured array of HIT_DTYPE records, (n,) or (n, max_hits) under "nearest_k" (synchronises).  A torch tensor on this instance's device
        goes through the device form and returns an (n * K, 64) uint8 tensor of the same records (K = max_hits under "nearest_k", otherwise 1),
        asynchronous on `stream` (default: torch's current stream).  Without the new arguments the call is the plain entry point's."""
        m, opts = self._query_options(mode, alpha, cull, max_hits, blend_threshold, seed)
        k = int(max_hits) if m == capi.MI_PT_QUERY_NEAREST_K else 1
        if opts is not None and not 1 <= k <= capi.MI_PT_QUERY_MAX_HITS:
            raise ValueError("query_rays: max_hits must lie in 1..%d" % capi.MI_PT_QUERY_MAX_HITS)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous()):
                raise ValueError("query_rays: a contiguous (n, 8) float32 device tensor is required")
            hits = torch.empty((rays.shape[0] * k, 64), dtype=torch.uint8, device=rays.device)
            if stream is None:
                stream = torch.cuda.current_stream(rays.device).cuda_stream
            if opts is None:
                _check_pt(self._l.mi_pt_query_rays_device(self._p, C.c_void_p(rays.data_ptr()), int(rays.shape[0]), m, C.c_void_p(hits.data_ptr()),
                                                          C.c_void_p(stream or 0)))
            else:
                _check_pt(self._l.mi_pt_query_rays_device_ex(self._p, C.c_void_p(rays.data_ptr()), int(rays.shape[0]), C.byref(opts),
                                                             C.c_void_p(hits.data_ptr()), C.c_void_p(stream or 0)))
            return hits
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError("query_rays: an (n, 8) float32 array is required")
        if opts is None:
            hits = np.zeros(rays.shape[0], HIT_DTYPE)
            _check_pt(self._l.mi_pt_query_rays(self._p, rays.ctypes.data_as(C.POINTER(capi.MiPtRay)), int(rays.shape[0]), m,
                                               hits.ctypes.data_as(C.POINTER(capi.MiPtRayHit))))
            return hits
        hits = np.zeros((rays.shape[0], k), HIT_DTYPE)
        _check_pt(self._l.mi_pt_query_rays_ex(self._p, rays.ctypes.data_as(C.POINTER(capi.MiPtRay)), int(rays.shape[0]), C.byref(opts),
                                              hits.ctypes.data_as(C.POINTER(capi.MiPtRayHit))))
        return hits if m == capi.MI_PT_QUERY_NEAREST_K else hits.reshape(-1)

    def pick(self, xy, mode="closest", alpha="opaque", cull="none", max_hits=1, blend_threshold=0.5, seed=0):
        """The closest hits of the camera rays through the continuous pixel positions `xy` ((n, 2) or one (x, y); (px + 0.5, py + 0.5) is the
        selection ray of pixel (px, py)) under the current frame info and size (mi_pt_pick).  Returns HIT_DTYPE records, one per position.
        With alpha / cull / mode="nearest_k" (as query_rays; mi_pt_pick_ex): alpha="cutoff", cull="material" names what the viewer sees at the
        pixel; "nearest_k" returns (n, max_hits) records, what lies under the cursor and behind that."""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        m, opts = self._query_options(mode, alpha, cull, max_hits, blend_threshold, seed)
        if opts is None:
            if m != capi.MI_PT_QUERY_CLOSEST:
                raise ValueError("pick: mode must be \"closest\" or \"nearest_k\"")
            hits = np.zeros(xy.shape[0], HIT_DTYPE)
            _check_pt(self._l.mi_pt_pick(self._p, xy.ctypes.data_as(C.POINTER(C.c_float)), int(xy.shape[0]), hits.ctypes.data_as(C.POINTER(capi.MiPtRayHit))))
            return hits
        k = int(max_hits) if m == capi.MI_PT_QUERY_NEAREST_K else 1
        if not 1 <= k <= capi.MI_PT_QUERY_MAX_HITS:
            raise ValueError("pick: max_hits must lie in 1..%d" % capi.MI_PT_QUERY_MAX_HITS)
        hits = np.zeros((xy.shape[0], k), HIT_DTYPE)
        _check_pt(self._l.mi_pt_pick_ex(self._p, xy.ctypes.data_as(C.POINTER(C.c_float)), int(xy.shape[0]), C.byref(opts),
                                        hits.ctypes.data_as(C.POINTER(capi.MiPtRayHit))))
        return hits if m == capi.MI_PT_QUERY_NEAREST_K else hits.reshape(-1)

    def read_depth(self):
        out = np.empty((self.height, self.width), dtype=np.float32)
        _check_pt(self._l.mi_pt_read_depth(self._p, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def denoise(self, iterations=5, sigma_color=0.6, sigma_normal=64.0, sigma_albedo=0.2):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check_pt(self._l.mi_pt_denoise(self._p, iterations, sigma_color, sigma_normal, sigma_albedo,
                                        out.ctypes.data_as(C.POINTER(C.c_float)), None))
        return out

    def denoise_svgf(self, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0, read=True, stream=None):
        """Variance-guided denoise (mi_pt_denoise_svgf); read=False leaves the result on the device (tonemap(source=1) picks it up)."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32) if read else None
        _check_pt(self._l.mi_pt_denoise_svgf(self._p, iterations, sigma_luminance, sigma_normal, sigma_depth,
                                             out.ctypes.data_as(C.POINTER(C.c_float)) if read else None, C.c_void_p(stream or 0)))
        return out

    def set_temporal(self, enable=True):
        """Motion vectors and temporal reprojection on / off (mi_pt_set_temporal): allocates the motion image, the history and the render
        nodes' previous matrices; every first-frame batch is then followed by the motion kernel.  Drops the history."""
        _check_pt(self._l.mi_pt_set_temporal(self._p, 1 if enable else 0))
        self.temporal = bool(enable)

    def read_first_hit(self):
        """(H, W, 4) float32 of the last first-frame batch: xyz = first-hit position (ray direction where the id is 0); view the last
        channel as uint32 for the id: renderNode + 1, 0 = miss / infinite plane, 0xffffffff = shadow-catcher path."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check_pt(self._l.mi_pt_read_first_hit(self._p, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def read_motion(self):
        """(H, W, 4) float32 motion image of the last first-frame batch: xy = motion in pixels (towards where the point was), z = the NDC
        depth it had, w = the id bits of read_first_hit."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check_pt(self._l.mi_pt_read_motion(self._p, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_vertex_motion(self, enable=True):
        """Skinned and morphed vertices carried in the motion image (mi_pt_set_vertex_motion): in force once set_temporal and set_deformation
        are too, in any order.  Records the first hit's triangle and keeps the deforming primitives' previous-pose positions.  Drops the history."""
        _check_pt(self._l.mi_pt_set_vertex_motion(self._p, 1 if enable else 0))

    def read_first_hit_triangle(self):
        """(H, W, 4) uint32 of the last first-frame batch: render primitive, triangle index inside it, the bits of the barycentrics b1, b2
        (view as float32; b0 = 1 - b1 - b2).  The first word is 0xffffffff where read_first_hit's id is 0 or 0xffffffff."""
        out = np.empty((self.height, self.width, 4), dtype=np.uint32)
        _check_pt(self._l.mi_pt_read_first_hit_triangle(self._p, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def read_previous_positions(self, prim):
        """(V, 3) float32: the positions render primitive `prim` had in the pose rendered before (mi_pt_read_previous_positions)."""
        n = int(self._scene.desc.contents.renderPrimitives[prim].vertexCount)
        out = np.zeros((n, 3), np.float32)
        _check_pt(self._l.mi_pt_read_previous_positions(self._p, int(prim), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def default_temporal(self, **fields):
        """MiPtTemporalParams with the library's defaults (mi_pt_default_temporal), fields overridden by name."""
        tp = capi.MiPtTemporalParams()
        self._l.mi_pt_default_temporal(C.byref(tp))
        for k, v in fields.items():
            setattr(tp, k, v)
        return tp

    def denoise_temporal(self, tp=None, read=True, stream=None, **fields):
        """SVGF with temporal reprojection (mi_pt_denoise_temporal), once per pose; tp = MiPtTemporalParams (default: default_temporal()),
        fields override members; read=False leaves the result on the device (tonemap(source=1) picks it up)."""
        if tp is None:
            tp = self.default_temporal()
        for k, v in fields.items():
            setattr(tp, k, v)
        out = np.empty((self.height, self.width, 4), dtype=np.float32) if read else None
        _check_pt(self._l.mi_pt_denoise_temporal(self._p, C.byref(tp), out.ctypes.data_as(C.POINTER(C.c_float)) if read else None, C.c_void_p(stream or 0)))
        return out

    def reset_history(self):
        _check_pt(self._l.mi_pt_reset_history(self._p))

    def tonemap(self, tm=None, source=0, dt_seconds=-1.0, **fields):
        """HDR -> display RGBA8 (H, W, 4 uint8) on the device; tm = MiTonemapperData (default: the reference's defaults with auto exposure
        off), fields override members (method may be a name from capi.TONEMAP_METHODS); source 1 = the last denoise() result."""
        if tm is None:
            tm = capi.MiTonemapperData()
            self._l.mi_pt_default_tonemapper(C.byref(tm), 0)
        for k, v in fields.items():
            setattr(tm, k, capi.TONEMAP_METHODS.index(v) if (k == "method" and isinstance(v, str)) else v)
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        _check_pt(self._l.mi_pt_tonemap(self._p, C.byref(tm), source, dt_seconds, out.ctypes.data_as(C.POINTER(C.c_uint8)), None))
        return out

    def stats(self):
        st = capi.MiPtStats()
        _check_pt(self._l.mi_pt_get_stats(self._p, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def memory(self):
        """mi_pt_get_memory: bytes of the scene (geometry, textures, acceleration structure), of the renderer (path state, queues, images) and of the device."""
        m = capi.MiPtMemory()
        _check_pt(self._l.mi_pt_get_memory(self._p, C.byref(m)))
        return {n: int(getattr(m, n)) for n, _ in m._fields_}

    def reset_stats(self):
        _check_pt(self._l.mi_pt_reset_stats(self._p))

    def enable_timing(self, on=True):
        _check_pt(self._l.mi_pt_enable_timing(self._p, 1 if on else 0))

    def frame_timing(self):
        t = capi.MiPtFrameTiming()
        _check_pt(self._l.mi_pt_get_frame_timing(self._p, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def close(self):
        if self._p:
            self._l.mi_pt_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeadlessRenderer:
    """Frame loop of the reference's headless path-trace mode: frameCount starts at -1 and is pre-incremented
    (src/renderer.cpp:1939-1977), frame 0 carries ePtFirstFrame and resets the sample counter
    (src/renderer_pathtracer.cpp:1502-1505, :1546-1549), totalSamples grows by numSamples per frame (:1401)."""

    def __init__(self, tracer, params):
        self.tracer = tracer
        self.params = params
        self.frame_count = -1
        self.total_samples = 0
        self._last_view_proj = None

    def reset_frame(self):
        self.frame_count = -1

    def set_frame_info(self, fi):
        """The camera of the next pose.  With the tracer's temporal reprojection on, prevMVP is filled with the viewProjMatrix of the
        pose before (the first pose: its own), as the reference's onRender keeps it (src/renderer.cpp:675-705); starts a new accumulation."""
        if self.tracer.temporal:
            fi.prevMVP[:] = self._last_view_proj if self._last_view_proj is not None else fi.viewProjMatrix[:]
            self._last_view_proj = fi.viewProjMatrix[:]
        self.tracer.set_frame_info(fi)
        self.reset_frame()

    def render(self, frames=1, stream=None, in_flight=1):
        """Advance `frames` frames; in_flight > 1 issues them in batches that share the wavefront launches."""
        done = 0
        while done < frames:
            batch = min(max(1, in_flight), frames - done)
            self.frame_count += 1
            if self.frame_count == 0:
                self.total_samples = 0
            p = self.params
            p.frameCount = self.frame_count
            p.totalSamples = self.total_samples
            p.flags = (p.flags & ~capi.MI_PT_FIRST_FRAME) | (capi.MI_PT_FIRST_FRAME if self.frame_count == 0 else 0)
            if batch == 1:
                self.tracer.render_frame(p, stream)
            else:
                self.tracer.render_frames(p, batch, stream)
            self.frame_count += batch - 1
            self.total_samples += p.numSamples * batch
            done += batch
