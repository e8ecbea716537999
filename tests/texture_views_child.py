"""Child process of tests/test_gpu_texture_views.py: renders debug views of a scene through caller-supplied camera rays in a fresh process, so that a
switch read at instance creation (MI_PT_DIAG_NO_QUADS=1: four texel gathers per bilinear tap instead of one footprint record) can differ from the
parent's.  argv: scene path, rays .npy (batches, SIDE * SIDE, 8), pixel angle, comma-separated view names, output .npy (batches, views, SIDE * SIDE, 3)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_gpu_texture_views as tv
    scene, rays_path, pixel_angle, views, out = sys.argv[1], sys.argv[2], float(sys.argv[3]), sys.argv[4].split(","), sys.argv[5]
    rays = np.load(rays_path)
    rig = tv.Rig(scene)
    try:
        res = np.stack([np.stack([rig.render(batch, v, pixel_angle) for v in views]) for batch in rays])
    finally:
        rig.close()
    np.save(out, res)
    print("texture views child ok", res.shape)


if __name__ == "__main__":
    main()
