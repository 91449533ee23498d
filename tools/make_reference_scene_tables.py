"""Generate tests/golden/reference_scene_tables.npz: the reference's own scenes (fr3_empty_world, xarm7_empty_world,
fr3_simple_pick_up) compiled by rcs_amd/mjcf.py, stored as numbers and names only, so that tests/test_host_logic.py
compares this repository's authored scenes against them without a reference checkout.

    python tools/make_reference_scene_tables.py REFERENCE_CHECKOUT

Keys: "<scene>/arrays/<table>" (every compiled table except geom_ / cam_ / mesh_), "<scene>/names/<kind>",
"<scene>/free_body/<field>" (the scene's single free body, if any; scalars as 0-d arrays).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
from rcs_amd.mjcf import compile_mjcf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_scene_tables.npz")
SCENES = ("fr3_empty_world", "xarm7_empty_world", "fr3_simple_pick_up")
NAMES = ("jnt_names", "actuator_names", "body_names", "geom_names")


def main(ref: str) -> None:
    out = {}
    for scene in SCENES:
        cm = compile_mjcf(os.path.join(ref, "assets", "scenes", scene, "scene.xml"))
        for k, a in cm.arrays.items():
            if not k.startswith(("geom_", "cam_", "mesh_")):
                out[f"{scene}/arrays/{k}"] = np.asarray(a)
        for n in NAMES:
            out[f"{scene}/names/{n}"] = np.array(getattr(cm, n), dtype=str)
        assert len(cm.free_bodies) <= 1, scene
        for fb in cm.free_bodies:
            for k, v in fb.items():
                out[f"{scene}/free_body/{k}"] = np.asarray(v)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
