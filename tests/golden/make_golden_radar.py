"""Generates tests/golden/radar_golden.npz by running the REFERENCE's own radar preprocessing functions (build container
only; /root/reference never travels).

/root/reference/Data_Preprocessing/Radar_data_preprocessing.py cannot be imported: at import time it lists the dataset
directory and starts a joblib pool over it (:24-43).  The three functions this path needs are pure numpy, so this script
parses the file with `ast`, picks `range_angle_map` (:7-13), `range_velocity_map` (:14-21) and `minmax` (:22-23) BY NAME and
executes exactly those definitions in a namespace holding numpy.  Nothing of the reference's text is stored.

Cubes: tests/radar_ref.py::cube(seed) for seeds 0 and 1, and the two tone cubes of radar_ref.TONES.  For each cube
  <key>_{ang,vel}_sample / _rows / _cols   the reference's normalised maps on the complex128 cast of the cube (the truth):
                                           every 61st element, row sums, column sums (float64)
  <key>_e32_{ang,vel}                      max |reference on the complex64 cube - truth| for that cube, under the numpy named
                                           in `numpy_version` (np.fft keeps complex64 only under numpy >= 2)
  e32_ang / e32_vel                        the largest of those over the two seeded cubes: the figure the tests' bars use (the
                                           tone cubes' own figures are larger for ang, smaller for vel, and only recorded)
Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_radar.py
"""
import ast
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np

from tests import radar_ref as rr

REF = "/root/reference/Data_Preprocessing/Radar_data_preprocessing.py"
NAMES = ["range_angle_map", "range_velocity_map", "minmax"]


def reference_functions():
    tree = ast.parse(open(REF).read(), filename=REF)
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in picked) == sorted(NAMES), [n.name for n in picked]
    ns = dict(np=np)
    exec(compile(ast.Module(body=picked, type_ignores=[]), REF, "exec"), ns)
    return ns


def cubes():
    out = {f"seed{sd}": rr.cube(sd) for sd in (0, 1)}
    out.update({f"tone{i}": rr.tone(*t) for i, t in enumerate(rr.TONES)})
    return out


def main():
    ns = reference_functions()

    def ref_maps(x):   # the reference's functions modify their argument in place (data -= mean): hand each a copy
        return (ns["minmax"](ns["range_angle_map"](x.copy())), ns["minmax"](ns["range_velocity_map"](x.copy())))

    out, e32, lines = {}, [0.0, 0.0], []
    for key, c in cubes().items():
        truth = ref_maps(c.astype(np.complex128))
        single = ref_maps(c)
        assert truth[0].dtype == np.float64 and single[0].dtype == np.float32, (truth[0].dtype, single[0].dtype)
        mine = rr.maps(c, np.complex128)
        for j, name in enumerate(("ang", "vel")):
            assert truth[j].shape == (256, 256)
            out[f"{key}_{name}_sample"], out[f"{key}_{name}_rows"], out[f"{key}_{name}_cols"] = rr.sample(truth[j])
            e = float(np.abs(single[j].astype(np.float64) - truth[j]).max())
            out[f"{key}_e32_{name}"] = np.float64(e)
            if key.startswith("seed"):
                e32[j] = max(e32[j], e)
            lines.append(f"{key} {name}: argmax {np.unravel_index(truth[j].argmax(), truth[j].shape)}, e32 {e:.3e}, "
                         f"max |radar_ref.maps - reference| {np.abs(mine[j] - truth[j]).max():.3e}")
    out["e32_ang"], out["e32_vel"] = np.float64(e32[0]), np.float64(e32[1])
    out["numpy_version"] = np.asarray(np.__version__)
    print("\n".join(lines))
    path = os.path.join(HERE, "radar_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote radar_golden.npz ({os.path.getsize(path)} bytes): e32_ang {e32[0]:.3e}, e32_vel {e32[1]:.3e}")


if __name__ == "__main__":
    main()
