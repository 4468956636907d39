"""Binary little-endian PLY for triangle meshes (numpy only): what voxblox's outputMeshAsPly / the server's final global mesh
write (coxgraph/src/server/visualizer/server_visualizer.cpp:20-142).  Vertices carry x y z (float), nx ny nz (float),
red green blue (uchar); faces are `list uchar int vertex_indices` triples.  read_ply reads back exactly this layout."""
import numpy as np

_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("i", "<i4", (3,))])


def write_ply(path, xyz, triangles, normals=None, rgb=None):
    """xyz float[n,3], triangles int[m,3] (indices into xyz), normals float[n,3] or None (zeros), rgb uint8[n,3] or None (zeros)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    n = len(xyz)
    if len(tri) and (tri.min() < 0 or tri.max() >= n):
        raise ValueError("triangle index out of range")
    v = np.zeros(n, _VERTEX)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        nr = np.asarray(normals, np.float32).reshape(n, 3)
        v["nx"], v["ny"], v["nz"] = nr[:, 0], nr[:, 1], nr[:, 2]
    if rgb is not None:
        c = np.asarray(rgb, np.uint8).reshape(n, 3)
        v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
    f = np.zeros(len(tri), _FACE)
    f["n"] = 3
    f["i"] = tri.astype(np.int32)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {n}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(tri)}\n"
              "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())


def read_ply(path):
    """-> dict(xyz, normals, rgb, triangles) of a file written by write_ply."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = nf = None
    for ln in lines:
        if ln.startswith("element vertex "):
            nv = int(ln.split()[2])
        elif ln.startswith("element face "):
            nf = int(ln.split()[2])
    if nv is None or nf is None:
        raise ValueError("PLY without vertex / face elements")
    v = np.frombuffer(data, _VERTEX, nv, end)
    f = np.frombuffer(data, _FACE, nf, end + nv * _VERTEX.itemsize)
    if nf and not np.all(f["n"] == 3):
        raise ValueError("only triangles are supported")
    return dict(xyz=np.stack([v["x"], v["y"], v["z"]], 1), normals=np.stack([v["nx"], v["ny"], v["nz"]], 1),
                rgb=np.stack([v["red"], v["green"], v["blue"]], 1), triangles=f["i"].astype(np.uint32).reshape(nf, 3))
