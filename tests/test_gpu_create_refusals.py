"""Every refusal of mi_pt_create's validation of a scene description (mi_pt_api.hip), one broken field at a time: the box's valid description
(plus one 1 x 1 texture, so that the texture checks have something to read) with one table pointer, count, index or size made wrong, and
MI_PT_COLLAPSE set to something that names no collapse.  Code and text of each refusal are compared with tests/golden/create_refusals.json,
recorded from the library as it stood before mi_pt_create was cut into phases; after each refusal the valid description still creates.
The check that a HIP device is visible comes first in mi_pt_create, which is why this needs the GPU.

`python tests/test_gpu_create_refusals.py OUT.json` (the repository root on PYTHONPATH) writes the refusals of the library in use."""
import copy
import ctypes as C
import json
import os
import sys

import pytest

from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "create_refusals.json")


class _Desc:
    """A copy of a scene's description whose tables can be edited: the structs are copied, what they point to (vertex streams) is the scene's."""

    def __init__(self, scene):
        src = scene.desc.contents
        self.d = capi.MiPtSceneDesc()
        C.memmove(C.byref(self.d), C.byref(src), C.sizeof(self.d))
        self.keep = [scene]
        for field, count, kind in (("materials", src.numMaterials, capi.MiGltfShadeMaterial), ("renderNodes", src.numRenderNodes, capi.MiGltfRenderNode),
                                   ("renderPrimitives", src.numRenderPrimitives, capi.MiPtRenderPrimitive)):
            table = (kind * count)()
            C.memmove(table, getattr(src, field), C.sizeof(table))
            setattr(self.d, field, C.cast(table, C.POINTER(kind)))
            self.keep.append(table)
        # one white texel that no material uses
        self.texel = (C.c_uint8 * 4)(255, 255, 255, 255)
        self.levels = (C.POINTER(C.c_uint8) * 1)(C.cast(self.texel, C.POINTER(C.c_uint8)))
        self.textures = (capi.MiPtTexture * 1)()
        self.textures[0].levels, self.textures[0].width, self.textures[0].height, self.textures[0].numLevels = self.levels, 1, 1, 1
        assert src.numTextures == 0
        self.d.textures, self.d.numTextures = self.textures, 1
        prim = self.d.renderPrimitives[0]
        self.indices = (C.c_uint32 * (3 * prim.triangleCount))()  # (an index table of the test's own to break)
        C.memmove(self.indices, prim.indices, C.sizeof(self.indices))


def _null(field, kind):
    return lambda s: setattr(s.d, field, C.POINTER(kind)())


def _set(field, value):
    return lambda s: setattr(s.d, field, value)


def _index_beyond(s):
    s.indices[4] = s.d.renderPrimitives[0].vertexCount
    s.d.renderPrimitives[0].indices = C.cast(s.indices, C.POINTER(C.c_uint32))


BREAKS = {
    "no materials": _set("numMaterials", 0),
    "no texture infos": _set("numTextureInfos", 0),
    "negative render-node count": _set("numRenderNodes", -1),
    "negative primitive count": _set("numRenderPrimitives", -1),
    "negative light count": _set("numLights", -1),
    "negative texture count": _set("numTextures", -1),
    "too many materials": _set("numMaterials", 65535 * 4 + 1),
    "null render nodes": _null("renderNodes", capi.MiGltfRenderNode),
    "null primitives": _null("renderPrimitives", capi.MiPtRenderPrimitive),
    "null lights": lambda s: (setattr(s.d, "numLights", 1), setattr(s.d, "lights", C.POINTER(capi.MiGltfLight)())),
    "null textures": _null("textures", capi.MiPtTexture),
    "null materials": _null("materials", capi.MiGltfShadeMaterial),
    "null texture infos": _null("textureInfos", capi.MiGltfTextureInfo),
    "node's material out of range": lambda s: setattr(s.d.renderNodes[0], "materialID", s.d.numMaterials),
    "material slot out of range": lambda s: setattr(s.d.materials[0], "emissiveTexture", s.d.numTextureInfos),
    "vertices without positions": lambda s: setattr(s.d.renderPrimitives[0], "positions", C.POINTER(C.c_float)()),
    "triangles without indices": lambda s: setattr(s.d.renderPrimitives[0], "indices", C.POINTER(C.c_uint32)()),
    "index beyond vertexCount": _index_beyond,
    "texture width 0": lambda s: setattr(s.textures[0], "width", 0),
    "texture height 65536": lambda s: setattr(s.textures[0], "height", 65536),
    "texture with no level": lambda s: setattr(s.textures[0], "numLevels", 0),
    "texture with 17 levels": lambda s: setattr(s.textures[0], "numLevels", 17),
    "MI_PT_COLLAPSE=typo": None,
}


def _create(desc):
    """(code, message) of mi_pt_create; an instance that was created is destroyed again"""
    lib, p, opts = capi.pt_lib(), C.c_void_p(), capi.MiPtCreateOptions()
    rc = lib.mi_pt_create(C.byref(desc), C.byref(opts), C.byref(p))
    if rc == 0:
        assert lib.mi_pt_destroy(p) == 0
        return {"rc": 0}
    assert not p.value
    return {"rc": rc, "message": lib.mi_pt_last_error().decode()}


def _refusal(name):
    scene = ptmod.Scene(os.path.join(ROOT, "assets", "Box.glb"))
    valid, broken = _Desc(scene), _Desc(scene)
    assert _create(valid.d) == {"rc": 0}
    if BREAKS[name] is None:
        os.environ["MI_PT_COLLAPSE"] = "typo"
        try:
            got = _create(broken.d)
        finally:
            del os.environ["MI_PT_COLLAPSE"]
    else:
        BREAKS[name](broken)
        got = _create(broken.d)
    assert got["rc"] != 0, (name, got)
    assert _create(valid.d) == {"rc": 0}  # the valid description still creates
    return copy.deepcopy(got)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_these_refusals(golden):
    assert sorted(golden) == sorted(BREAKS)


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_refusal_is_the_one_recorded_before_create_was_cut_into_phases(name, golden):
    got = _refusal(name)
    print(name, json.dumps(got))
    assert got == golden[name]


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({name: _refusal(name) for name in sorted(BREAKS)}, f, indent=1, sort_keys=True)
        f.write("\n")
