"""Generate tests/golden/denoise_var_cornell_64x64.npz from the CPU oracle alone (about a minute):

    python tests/golden/gen_denoise_var_golden.py

Two independent 2-sample half-frames of the cornell box at 64x64 (`half_a`, `half_b`, linear RGB (3, 4096)
float64): what srt_denoise_var is given.  They are judged against the 64-sample `ref` of
denoise_cornell_64x64.npz (gen_denoise_golden.py), which is not repeated here.  The camera jitter comes
from numpy Generators and the Monte-Carlo draws from the oracle's restatement of the device stream, so the
file depends on neither numpy's global RNG nor a GPU:

    half_a = render_linear(cornell(64, 64), default_rng(3).random((2, 4, 4096)), stream=DeviceStream(13))[0]
    half_b = render_linear(cornell(64, 64), default_rng(4).random((2, 4, 4096)), stream=DeviceStream(17))[0]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

W = H = 64
HALF_A = {"spp": 2, "jitter_seed": 3, "stream_seed": 13}
HALF_B = {"spp": 2, "jitter_seed": 4, "stream_seed": 17}


def frame(sc, spec):
    import sightpy_oracle as O

    jit = np.random.default_rng(spec["jitter_seed"]).random((spec["spp"], 4, W * H))
    return O.render_linear(sc, jit, stream=O.DeviceStream(spec["stream_seed"]))[0]


def main():
    import scenes

    sc = scenes.cornell(W, H)
    out = Path(__file__).resolve().parent / "denoise_var_cornell_64x64.npz"
    np.savez_compressed(out, half_a=frame(sc, HALF_A), half_b=frame(sc, HALF_B), width=W, height=H,
                        spp_a=HALF_A["spp"], spp_b=HALF_B["spp"],
                        a_jitter_seed=HALF_A["jitter_seed"], a_stream_seed=HALF_A["stream_seed"],
                        b_jitter_seed=HALF_B["jitter_seed"], b_stream_seed=HALF_B["stream_seed"])
    print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
