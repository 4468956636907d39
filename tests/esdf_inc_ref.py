"""Plain numpy statement of the incremental ESDF update (classify, raise, lower) on the wire arrays of
Layer.download(), and the seeded TSDF edits the incremental tests apply (tests/test_esdf_inc_cpu.py, tests/test_gpu_esdf_inc.py).
Shares no code with the kernels; the dense scatter / gather is tests/submap_ref.py's."""
import numpy as np

import submap_cases
from submap_ref import Dense, F32, OFFSETS, _shift, fields


def _keys(idx):
    return [tuple(int(v) for v in r) for r in np.asarray(idx).reshape(-1, 3)]


class IncrementalEsdfRef:
    """state: the ESDF words per block, as the engine keeps them; update(idx, vox) -> words uint32[n,4096,3] in idx order"""

    def __init__(self, voxel_size, max_distance_m, min_distance_m, default_distance_m, min_weight):
        self.vs, self.max_d, self.min_d = F32(voxel_size), F32(max_distance_m), F32(min_distance_m)
        self.default_d, self.min_w = F32(default_distance_m), F32(min_weight)
        self.state = {}
        self.stats = {}

    def update(self, idx, vox):
        keys = _keys(idx)
        rebuilt = any(k not in set(keys) for k in self.state)   # the TSDF lost blocks
        if rebuilt:
            self.state = {}
        stored = np.zeros((len(keys), 4096, 3), np.uint32)
        for i, k in enumerate(keys):
            if k in self.state:
                stored[i] = self.state[k]
        # classify
        d, w = fields(vox)
        s_d, s_obs, s_fixed = stored[..., 0].copy().view(F32), stored[..., 1].copy().view(F32) > 0, stored[..., 2] != 0
        with np.errstate(invalid="ignore"):
            obs = ~(w < self.min_w)
            fixed = obs & (np.abs(d) < self.min_d)
            init = np.where(d > 0, self.default_d, -self.default_d).astype(F32)
            free = obs & ~fixed
            keep = free & s_obs & ~s_fixed & ((s_d > 0) == (d > 0))
        e = np.where(fixed, d, np.where(keep, s_d, init)).astype(F32)
        e[~obs] = 0.0
        words = self._words(e, obs, fixed)
        dirty = (words != stored).any(axis=(1, 2))
        n_reset = 0
        if len(keys) and dirty.any():
            G = Dense(idx)
            E, O = G.scatter(e, F32(0)), G.scatter(obs, False)
            M = G.scatter(free, False)[1:-1, 1:-1, 1:-1]
            steps = {1: F32(1.0) * self.vs, 2: np.sqrt(F32(2.0)) * self.vs, 3: np.sqrt(F32(3.0)) * self.vs}
            inner = E[1:-1, 1:-1, 1:-1]
            # raise: a free voxel off its init value needs a neighbour that offers exactly that value
            while True:
                with np.errstate(invalid="ignore"):
                    init_d = np.where(inner > 0, self.default_d, -self.default_d).astype(F32)
                    need = M & (inner != init_d)
                    supported = np.zeros(inner.shape, bool)
                    for o in OFFSETS:
                        step = steps[abs(o[0]) + abs(o[1]) + abs(o[2])]
                        src = _shift(E, o)
                        ok = _shift(O, o) & (np.abs(src) < self.max_d)
                        cand = np.where(src > 0, src + step, src - step).astype(F32)
                        supported |= ok & (cand == inner)
                drop = need & ~supported
                if not drop.any():
                    break
                n_reset += int(drop.sum())
                inner[drop] = init_d[drop]
            # lower: the batch's relaxation from there
            while True:
                before = inner.copy()
                for o in OFFSETS:
                    step = steps[abs(o[0]) + abs(o[1]) + abs(o[2])]
                    src = _shift(E, o)
                    with np.errstate(invalid="ignore"):
                        ok = _shift(O, o) & (np.abs(src) < self.max_d) & M
                        pos = ok & (src > 0)
                    lo = np.where(pos, src + step, F32(np.inf)).astype(F32)
                    hi = np.where(ok & ~pos, src - step, F32(-np.inf)).astype(F32)
                    np.copyto(inner, lo, where=inner > lo)
                    np.copyto(inner, hi, where=inner < hi)
                if np.array_equal(before.view(np.uint32), inner.view(np.uint32)):
                    break
            e = G.gather(E)
            words = self._words(e, obs, fixed)
        self.state = {k: words[i] for i, k in enumerate(keys)}
        self.stats = dict(rebuilt=int(rebuilt), n_dirty_blocks=int(dirty.sum()), n_reset_voxels=n_reset)
        return words

    @staticmethod
    def _words(e, obs, fixed):
        w = np.zeros(e.shape + (3,), np.uint32)
        w[..., 0] = np.ascontiguousarray(e, F32).view(np.uint32)
        w[..., 1] = np.where(obs, F32(1.0), F32(0.0)).astype(F32).view(np.uint32)
        w[..., 2] = fixed.astype(np.uint32)
        return w


# ---- seeded edits: each is an upload (block indices, words, action) into the TSDF layer ---------------------------------------
EDITS = ("overwrite", "new_blocks", "zero_weights", "negate_box", "merge")


def uploaded_seeds(n, propagating):
    """the first n seeds whose case is an uploaded layer (the fused family integrates frames and has no arrays to edit)"""
    out, s = [], 0
    while len(out) < n:
        if submap_cases.case(s, propagating=propagating)[1] is not None:
            out.append(s)
        s += 1
    return out


def start_half(c):
    """the half of a case's blocks the sequence starts from, and the rest"""
    rng = np.random.default_rng(c[5]["seed"] + 4242)
    p = rng.permutation(len(c[1]))
    return np.sort(p[: (len(p) + 1) // 2]), np.sort(p[(len(p) + 1) // 2:])


def _centres(idx, voxel):
    return ((idx[:, None, :].astype(np.int64) * 16 + submap_cases.LOC[None]).astype(np.float64) + 0.5) * float(F32(voxel))


def make_edit(kind, c, cur_idx, cur_vox, seed):
    """-> (idx int32[m,3], vox uint32[m,4096,3], action) given the layer's current download (cur_idx, cur_vox)"""
    voxel, idx_all, vox_all = c[0], c[1], c[2]
    rng = np.random.default_rng(31337 * seed + EDITS.index(kind))
    n = len(cur_idx)
    if kind == "overwrite":       # a random block subset takes another seed's field
        other = submap_cases.reading_case(c, seed + 77)
        pick = np.flatnonzero(rng.random(len(idx_all)) < 0.3)
        if len(pick) == 0:
            pick = np.array([0])
        have = set(_keys(cur_idx))
        pick = np.array([i for i in pick if tuple(int(v) for v in idx_all[i]) in have] or [_keys(idx_all).index(_keys(cur_idx)[0])])
        return idx_all[pick], other[2][pick], 0
    if kind == "new_blocks":      # the rest of the case: new pool blocks, a pool that grows
        rest = start_half(c)[1]
        return idx_all[rest], vox_all[rest], 0
    if kind in ("zero_weights", "negate_box"):
        cen = _centres(cur_idx, voxel)
        centre = cen[rng.integers(n), rng.integers(4096)]
        vox = cur_vox.copy()
        if kind == "zero_weights":
            m = np.linalg.norm(cen - centre, axis=-1) < rng.uniform(4, 12) * voxel
            vox[..., 1][m] = 0
        else:
            m = (np.abs(cen - centre) < rng.uniform(3, 10, 3) * voxel).all(axis=-1)
            vox[..., 0][m] ^= np.uint32(0x80000000)
        touched = m.any(axis=1)
        if not touched.any():
            touched[0] = True
        return cur_idx[touched], vox[touched], 0
    other = submap_cases.reading_case(c, seed + 123)   # merge: a second layer over a block subset, mergeVoxelAIntoVoxelB
    pick = np.flatnonzero(rng.random(len(idx_all)) < 0.4)
    if len(pick) == 0:
        pick = np.array([0])
    return idx_all[pick], other[2][pick], 1


def apply_upload(cur_idx, cur_vox, idx, vox, action):
    """numpy cox_layer_upload (action 0 overwrite, 1 merge) -> (idx, vox) in download order"""
    blocks = {k: cur_vox[i] for i, k in enumerate(_keys(cur_idx))}
    for i, k in enumerate(_keys(idx)):
        if action == 1 and k in blocks:
            b = blocks[k].copy()
            ad, aw = fields(vox[i])
            bd, bw = fields(b)
            cw = (aw + bw).astype(F32)
            with np.errstate(invalid="ignore", divide="ignore"):
                nd = ((ad * aw + bd * bw) / cw).astype(F32)
            m = cw > 0
            b[..., 0][m] = nd.view(np.uint32)[m]
            b[..., 1][m] = cw.view(np.uint32)[m]
            blocks[k] = b
        else:
            blocks[k] = vox[i].copy()
    ks = sorted(blocks, key=lambda k: (k[2], k[1], k[0]))
    return np.array(ks, np.int32).reshape(-1, 3), np.stack([blocks[k] for k in ks]) if ks else np.zeros((0, 4096, 3), np.uint32)
