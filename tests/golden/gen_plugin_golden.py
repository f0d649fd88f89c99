"""Generate the plugin fixtures tests/golden/plugin_{texture,light,both}_48x36_d3_s2.npz by running
the REFERENCE implementation on the scenes of tests/plugin_scenes.py (user texture and Light
subclasses defined against the reference's own base classes), through gen_golden.py's harness:

    python tests/golden/gen_plugin_golden.py

Runs where the reference is available (see gen_golden.py); the tests read only the .npz files.
"""
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))

from gen_golden import import_reference, render_golden  # noqa: E402

W, H, DEPTH, SPP, SEED = 48, 36, 3, 2, 11


def main():
    sp = import_reference()
    import plugin_scenes

    for kind in plugin_scenes.KINDS:
        scene = plugin_scenes.scene(kind, W, H, DEPTH, sp=sp)
        calls = plugin_scenes.classes(sp).calls
        for k in calls:
            calls[k] = 0
        lin, u8, hits, nears, counts = render_golden(sp, scene, SPP, SEED)
        name = "plugin_%s_%dx%d_d%d_s%d" % (kind, W, H, DEPTH, SPP)
        np.savez_compressed(OUT / (name + ".npz"), rgb=lin.astype("f8"), srgb8=u8, seed=SEED, spp=SPP, width=W,
                            height=H, depth=DEPTH)
        print(name, "rays per depth", counts.tolist(), "rgb mean", lin.mean(), "user calls", dict(calls))


if __name__ == "__main__":
    main()
