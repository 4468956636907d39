"""The GPU mesh clean-up (coxgraph_amd/csrc/cox_meshclean.hip) against the float64 numpy reference (tests/meshclean_ref.py).

Compared exactly: every count, the triangle arrays, the vertex order, the cell partition (through the re-indexed triangles and
the vertex count), colours, which vertices moved, and -- bit for bit -- two runs of the same call.  Compared within a tolerance:
positions and normals, whose sums the GPU takes in float32.  The tolerance of an input is 8 times the largest deviation of the
float32 restatement (the same rules with float32 sums) from the float64 reference on that input, never less than one float32 ulp
of the largest value compared; the factor covers differences that do not come from the summation order (divide, square root).
It never comes from the GPU's own result.

`PYTHONPATH=.:tests python tests/test_gpu_meshclean.py` prints the measured deviations below (no GPU needed).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import meshclean_cases as K
import meshclean_ref as R
from coxgraph_amd import mesh_io
from coxgraph_amd.capi import ConnectedMesh, CoxError, MeshLayer
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest |float32 restatement - float64 reference| per input, measured on the CPU with the function measure() below:
# (Taubin 1 iteration [m], Taubin 100 iterations [m], cluster positions [m], cluster normals, vertex normals).
# Clustering uses the cell size of CELL below.  The smoothing tests print the largest motion next to the error, for scale.
MEASURED = {
    "grid48": (1.074e-06, 3.220e-06, 6.888e-07, 2.533e-07, 9.570e-08),
    "grid24_far": (1.304e-05, 8.621e-05, 5.086e-06, 1.043e-07, 1.047e-07),
    "fan70": (1.088e-07, 1.546e-07, 5.960e-08, 9.418e-08, 3.044e-07),
    "sphere": (5.336e-07, 1.518e-06, 1.589e-07, 1.232e-07, 1.105e-07),
    "dense": (5.542e-08, 2.150e-07, 1.311e-07, 2.240e-07, 9.105e-08),
    "dups": (8.677e-07, 3.951e-06, 2.384e-07, 1.906e-07, 9.828e-08),
}
CELL = {"grid48": 0.25, "grid24_far": 0.25, "fan70": 0.5, "sphere": 0.3, "dense": 0.25, "dups": 0.25}


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "grid48":      # 2 304 vertices, 4 418 triangles, 26 508 directed edges: more than one 2 048-element tile each
        return K.grid(48, 0.1, noise=0.02, seed=3, offset=(-2.0, -3.1, 5.0))
    if name == "grid24_far":  # about 100 m out, negative coordinates
        return K.grid(24, 0.1, noise=0.02, seed=4, offset=(100.3, -99.7, -3.2))
    if name == "fan70":       # one neighbour row of 71 entries
        return K.fan(70)
    if name == "sphere":
        return K.icosphere(3, 1.5, center=(0.3, -0.2, 1.0), noise=0.01)
    if name == "dense":       # 576 vertices within 0.46 m: four cells of 0.25 m gather 144 members each
        return K.grid(24, 0.02, noise=0.005, seed=5)
    if name == "dups":        # copies of triangles more than a sort tile (2 048) away from their originals, rotated and flipped
        m = dict(K.grid(48, 0.1, noise=0.02, seed=6))
        t = m["triangles"]
        m["triangles"] = np.concatenate([t, t[:300][:, [1, 2, 0]], t[100:200][:, [0, 2, 1]], t[4000:4100][:, [2, 0, 1]], t[:50]])
        return m
    raise KeyError(name)


CASES = ["grid48", "grid24_far", "fan70", "sphere", "dense", "dups"]


def _ulp(a):
    return float(np.spacing(np.float32(np.max(np.abs(a))))) if np.size(a) else 0.0


@functools.lru_cache(maxsize=None)
def references(name):
    """The float64 reference of every operation on one input, computed once and shared."""
    m = case(name)
    return dict(clean=R.clean(m), smooth1=R.smooth_taubin(m, 1), smooth100=R.smooth_taubin(m, 100), cluster=R.simplify_clustering(m, CELL[name])[0],
                normals=R.compute_normals(m))


def measure(name):
    m, ref = case(name), references(name)
    c32 = R.simplify_clustering(m, CELL[name], np.float32)[0]
    dev = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b))) if np.size(b) else 0.0  # noqa: E731
    return (dev(R.smooth_taubin(m, 1, dtype=np.float32), ref["smooth1"]), dev(R.smooth_taubin(m, 100, dtype=np.float32), ref["smooth100"]),
            dev(c32["xyz"], ref["cluster"]["xyz"]), dev(c32["normals"], ref["cluster"]["normals"]), dev(R.compute_normals(m, np.float32), ref["normals"]))


def _tol(name, k, compared):
    return max(8.0 * MEASURED[name][k], _ulp(compared))


def _upload(hip, m):
    return ConnectedMesh.from_arrays(hip, m["xyz"], m["triangles"], m["normals"], m["rgb"])


def _same_bits(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("xyz", "normals", "rgb", "triangles"))


def _twice(hip, m, op):
    """op on two fresh uploads of m: -> (result of op, downloaded mesh), after checking that both runs agree bit for bit."""
    out = []
    for _ in range(2):
        c = _upload(hip, m)
        r = op(c)
        out.append((r, c.download(), c.size))
        c.close()
    assert out[0][0] == out[1][0] or isinstance(out[0][0], float)
    assert _same_bits(out[0][1], out[1][1]), "two runs differ"
    assert out[0][2] == (len(out[0][1]["xyz"]), len(out[0][1]["triangles"]))
    return out[0][0], out[0][1]


def _check_clean(g, removed, ref):
    want, want_removed = ref
    assert removed == want_removed
    assert np.array_equal(g["triangles"], want["triangles"])
    assert _same_bits(g, dict(want, xyz=want["xyz"].astype(np.float32), normals=want["normals"].astype(np.float32)))


@pytest.mark.parametrize("name", CASES)
def test_clean(hip, name):
    removed, g = _twice(hip, case(name), lambda c: c.clean())
    _check_clean(g, removed, references(name)["clean"])
    if name == "dups":
        assert removed == (0, 450, 0)  # the 300 + 100 rotated and the 50 plain copies; the 100 flipped ones stay


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("iterations", [0, 1, 100])
def test_smooth_taubin(hip, name, iterations):
    m = case(name)
    ms, g = _twice(hip, m, lambda c: c.smooth_taubin(iterations))
    for k in ("normals", "rgb", "triangles"):
        assert np.array_equal(g[k], m[k]), k
    if iterations == 0:
        assert np.array_equal(g["xyz"].view(np.uint32), m["xyz"].view(np.uint32)) and ms == 0.0
        return
    want = references(name)["smooth1" if iterations == 1 else "smooth100"]
    err, tol = np.max(np.abs(g["xyz"] - want)), _tol(name, 0 if iterations == 1 else 1, want)
    print(f"{name} x{iterations}: max |gpu - f64| {err:.3e}, tolerance {tol:.3e}, largest motion {np.max(np.abs(want - m['xyz'])):.3e}, {ms:.3f} ms")
    assert err <= tol
    assert np.array_equal(np.any(g["xyz"] != m["xyz"], axis=1), np.any(want.astype(np.float32) != m["xyz"], axis=1))
    assert ms > 0.0


@pytest.mark.parametrize("name", CASES)
def test_simplify_clustering(hip, name):
    m = case(name)
    size, g = _twice(hip, m, lambda c: c.simplify_clustering(CELL[name]))
    want = references(name)["cluster"]
    assert size == (len(want["xyz"]), len(want["triangles"])) == (len(g["xyz"]), len(g["triangles"]))
    assert np.array_equal(g["triangles"], want["triangles"]) and np.array_equal(g["rgb"], want["rgb"])
    for key, k in (("xyz", 2), ("normals", 3)):
        err, tol = (np.max(np.abs(g[key] - want[key])) if len(g[key]) else 0.0), _tol(name, k, want[key])
        print(f"{name} {key}: max |gpu - f64| {err:.3e}, tolerance {tol:.3e}, {size[0]} of {len(m['xyz'])} vertices")
        assert err <= tol
    if name == "dense":
        assert np.max(R.partition(m["xyz"], CELL[name])[2]) > 64


@pytest.mark.parametrize("name", CASES)
def test_compute_normals(hip, name):
    m = case(name)
    _, g = _twice(hip, m, lambda c: c.compute_normals())
    for k in ("xyz", "rgb", "triangles"):
        assert np.array_equal(g[k], m[k]), k
    want = references(name)["normals"]
    err, tol = np.max(np.abs(g["normals"] - want)), _tol(name, 4, want)
    print(f"{name}: max |gpu - f64| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


def test_normals_of_the_analytic_sphere_are_radial(hip):
    center = np.array([0.4, -1.0, 2.0])
    s = K.icosphere(3, 2.0, center=center)
    c = _upload(hip, s)
    c.compute_normals()
    n = c.download()["normals"].astype(np.float64)
    u = s["xyz"].astype(np.float64) - center
    cos = np.einsum("ij,ij->i", n, u / np.linalg.norm(u, axis=1)[:, None])
    assert cos.min() > 0.9999 and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)


def _close(got, want, want32):
    """got within 8 x (float32 restatement - float64 reference), at least one ulp: the rule of the module docstring, measured in place."""
    if not np.size(want):
        return got.shape == want.shape
    return got.shape == want.shape and np.max(np.abs(got - want)) <= max(8 * np.max(np.abs(want32.astype(np.float64) - want)), _ulp(want))


def _all_ops(hip, m, cell=0.5):
    """Every operation on a small mesh against the reference; -> the size after clustering."""
    removed, g = _twice(hip, m, lambda c: c.clean())
    _check_clean(g, removed, R.clean(m))
    for it in (0, 1, 3):
        _, g = _twice(hip, m, lambda c: c.smooth_taubin(it))
        want = R.smooth_taubin(m, it)
        assert _close(g["xyz"], want, R.smooth_taubin(m, it, dtype=np.float32))
        assert np.array_equal(np.any(g["xyz"] != m["xyz"], axis=1), np.any(want.astype(np.float32) != m["xyz"], axis=1))
    _, g = _twice(hip, m, lambda c: c.compute_normals())
    assert _close(g["normals"], R.compute_normals(m), R.compute_normals(m, np.float32))
    size, g = _twice(hip, m, lambda c: c.simplify_clustering(cell))
    want, w32 = R.simplify_clustering(m, cell)[0], R.simplify_clustering(m, cell, np.float32)[0]
    assert size == (len(want["xyz"]), len(want["triangles"])) and np.array_equal(g["triangles"], want["triangles"]) and np.array_equal(g["rgb"], want["rgb"])
    assert _close(g["xyz"], want["xyz"], w32["xyz"]) and _close(g["normals"], want["normals"], w32["normals"])
    return size


def test_small_meshes(hip):
    empty = R.mesh(np.zeros((0, 3)), np.zeros((0, 3)))
    assert _all_ops(hip, empty) == (0, 0)
    one = R.mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 2, 0]], rgb=[[10, 20, 30], [40, 50, 60], [70, 80, 90]], normals=[[0, 0, 1]] * 3)
    assert _all_ops(hip, one) == (3, 1)
    tetra = R.mesh(K.TETRA_XYZ, K.TETRA_TRI, rgb=np.arange(12).reshape(4, 3))
    assert _all_ops(hip, tetra) == (4, 4)
    assert _all_ops(hip, tetra, cell=4.0) == (0, 0)  # one cell: every triangle degenerates, every vertex goes
    isolated = R.mesh(np.concatenate([K.TETRA_XYZ, [[5, 5, 5], [-1, 0, 0]]]), K.TETRA_TRI + 0, rgb=np.arange(18).reshape(6, 3))
    assert _all_ops(hip, isolated) == (4, 4)
    only_vertices = R.mesh(K.TETRA_XYZ, np.zeros((0, 3)))
    assert _all_ops(hip, only_vertices) == (0, 0)
    xyz = np.arange(18, dtype=np.float32).reshape(6, 3) ** 1.5
    degenerate = R.mesh(xyz, [[4, 4, 1], [5, 1, 3], [3, 5, 1], [2, 3, 2], [0, 0, 0], [1, 5, 3]], rgb=np.arange(18).reshape(6, 3))
    c = _upload(hip, degenerate)
    assert c.clean() == (3, 1, 3) and c.size == (3, 2)
    _all_ops(hip, degenerate, cell=1.0)


def test_bad_arguments_and_index_range(hip):
    m = case("fan70")
    with pytest.raises(CoxError) as e:
        ConnectedMesh.from_arrays(hip, m["xyz"], [[0, 1, len(m["xyz"])]])
    assert e.value.status == -5
    c = _upload(hip, m)
    before = c.download()
    for bad in (lambda: c.smooth_taubin(-1), lambda: c.smooth_taubin(3, float("nan")), lambda: c.smooth_taubin(3, 0.5, float("inf")),
                lambda: c.simplify_clustering(0.0), lambda: c.simplify_clustering(-0.1), lambda: c.simplify_clustering(float("nan")),
                lambda: c.simplify_clustering(float("inf"))):
        with pytest.raises(CoxError) as e:
            bad()
        assert e.value.status == -1
    # the fan spans 2 m: 2^21 cells need a cell below 9.6e-7 m
    with pytest.raises(CoxError) as e:
        c.simplify_clustering(9e-7)
    assert e.value.status == -5
    with pytest.raises(R.IndexRange):
        R.partition(m["xyz"], 9e-7)
    assert c.simplify_clustering(1.1e-6)[0] == len(m["xyz"])  # below the limit: every vertex its own cell, reordered by cell
    assert _same_bits(before, _upload(hip, m).download())


def test_global_mesh_of_two_submaps_through_the_whole_chain(hip):
    """tests/test_gpu_mesh.py's two submaps, welded on the device, then clean -> smooth(10) -> cluster(0.05) -> normals with the mesh
    staying on the device; every stage against the reference applied to the stage before it.  The input only exists on the GPU, so
    the float32 deviation behind the tolerance is measured here, on the reference's side, as for the constants above."""
    voxel = 0.10
    a, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    b, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(70, 150, 10), subsample=4, capacity_blocks=8192)
    th = np.radians(3.0)
    T = np.stack([np.array([np.cos(th / 2), 0, 0, np.sin(th / 2), 0.07, -0.03, 0.01], np.float32), np.array([1, 0, 0, 0, 0, 0, 0], np.float32)])
    parts = [MeshLayer.from_layer(hip, a, 1.0), MeshLayer.from_layer(hip, b, 1.0)]
    welded = MeshLayer.connected(hip, parts, T, 0.5 * voxel)
    c = MeshLayer.connected_mesh(hip, parts, T, 0.5 * voxel)
    s0 = c.download()
    assert _same_bits(s0, welded) and c.size[1] > 1000

    removed = c.clean()
    s1 = c.download()
    _check_clean(s1, removed, R.clean(s0))
    print(f"weld {len(s0['xyz'])} vertices {len(s0['triangles'])} triangles, clean removed {removed}")

    assert c.smooth_taubin(10) > 0
    s2 = c.download()
    want = R.smooth_taubin(s1, 10)
    tol = max(8 * np.max(np.abs(R.smooth_taubin(s1, 10, dtype=np.float32) - want)), _ulp(want))
    print(f"smooth: max |gpu - f64| {np.max(np.abs(s2['xyz'] - want)):.3e}, tolerance {tol:.3e}")
    assert np.max(np.abs(s2["xyz"] - want)) <= tol and np.array_equal(s2["triangles"], s1["triangles"]) and np.array_equal(s2["normals"], s1["normals"])

    size = c.simplify_clustering(0.05)
    s3 = c.download()
    want = R.simplify_clustering(s2, 0.05)[0]
    w32 = R.simplify_clustering(s2, 0.05, np.float32)[0]
    assert size == (len(want["xyz"]), len(want["triangles"])) and size[0] <= len(s2["xyz"])
    assert np.array_equal(s3["triangles"], want["triangles"]) and np.array_equal(s3["rgb"], want["rgb"])
    for key in ("xyz", "normals"):
        tol = max(8 * np.max(np.abs(w32[key] - want[key])), _ulp(want[key]))
        print(f"cluster {key}: max |gpu - f64| {np.max(np.abs(s3[key] - want[key])):.3e}, tolerance {tol:.3e}")
        assert np.max(np.abs(s3[key] - want[key])) <= tol

    c.compute_normals()
    s4 = c.download()
    want = R.compute_normals(s3)
    tol = max(8 * np.max(np.abs(R.compute_normals(s3, np.float32) - want)), _ulp(want))
    print(f"normals: max |gpu - f64| {np.max(np.abs(s4['normals'] - want)):.3e}, tolerance {tol:.3e}")
    assert np.max(np.abs(s4["normals"] - want)) <= tol
    assert np.array_equal(s4["xyz"], s3["xyz"]) and np.array_equal(s4["triangles"], s3["triangles"])
    c.close()


def test_cpp_global_mesh_cleanup_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "meshclean_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "meshclean_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    for name in ("global_mesh_clean.ply", "global_mesh_loop.ply"):
        g = mesh_io.read_ply(str(tmp_path / name))
        m = R.mesh(g["xyz"], g["triangles"])
        assert len(g["triangles"]) > 100 and R.clean(m)[1] == (0, 0, 0)
        # the normals in the file are the ones compute_normals gives for the positions in the file
        assert _close(g["normals"], R.compute_normals(m), R.compute_normals(m, np.float32))


if __name__ == "__main__":
    for n in CASES:
        print(f'    "{n}": ({", ".join(f"{v:.3e}" for v in measure(n))}),')
