"""The stream plans of a tight queue budget (COX_QUEUES = 1 ... 4: no input stream, three streams or fewer -- cox_plan.hpp) against
the plan of ample queues: same frames, same layer, bit for bit."""
import functools

import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, Integrator

pytestmark = pytest.mark.gpu

N_FRAMES, SUB = 12, 8   # 12 frames > 6 frame slots and staging sets: every buffer set is reused


@functools.lru_cache(maxsize=None)
def frames():
    out = []
    for t in range(N_FRAMES):
        T, p, c, _ = synth.make_frame(t)
        out.append((T, np.ascontiguousarray(p[::SUB]), np.ascontiguousarray(c[::SUB])))
    return out


_reference = {}


def reference(hip, monkeypatch, method, voxel):
    """(stats, block indices, voxels) of the frames fed one at a time through the synchronous host path to an integrator planned for
    16 queues (today's streams); computed once per (method, voxel) and left alone."""
    if (method, voxel) not in _reference:
        layer = Layer(hip, voxel, capacity_blocks=32768)
        monkeypatch.setenv("COX_QUEUES", "16")
        integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **synth.integrator_overrides(voxel)), method)
        monkeypatch.delenv("COX_QUEUES")
        for T, p, c in frames():
            integ.integrate_points(T, p, c)
        idx, vox = layer.download()
        idx.setflags(write=False)
        vox.setflags(write=False)
        _reference[(method, voxel)] = (integ.last_stats(), idx, vox)
    return _reference[(method, voxel)]


def planned_for(hip, monkeypatch, queues, method, voxel):
    layer = Layer(hip, voxel, capacity_blocks=32768)
    monkeypatch.setenv("COX_QUEUES", str(queues))   # read when the integrator is created
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **synth.integrator_overrides(voxel)), method)
    monkeypatch.delenv("COX_QUEUES")
    return layer, integ


def same(layer, integ, ref):
    stats, idx, vox = ref
    assert integ.last_stats() == stats
    ja, va = layer.download()
    assert np.array_equal(ja, idx) and np.array_equal(va, vox)


@pytest.mark.parametrize("queues", [1, 2, 3, 4])
@pytest.mark.parametrize("method,voxel", [("merged", 0.05), ("simple", 0.05), ("merged", 0.02), ("fast", 0.05)])
def test_tight_queue_budgets_give_the_same_layer(hip, monkeypatch, method, voxel, queues):
    """Resident frames enqueued back to back on the streams of a budget of 1, 2, 3 or 4 queues."""
    import torch
    ref = reference(hip, monkeypatch, method, voxel)
    layer, integ = planned_for(hip, monkeypatch, queues, method, voxel)
    dev = [(T, torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda()) for T, p, c in frames()]
    torch.cuda.synchronize()
    for T, xyz, rgba in dev:
        integ.integrate_points_dev(T, xyz.data_ptr(), rgba.data_ptr(), xyz.shape[0])
    integ.sync()
    same(layer, integ, ref)


@pytest.mark.parametrize("method", ["merged", "fast"])
def test_pinned_host_clouds_without_an_input_stream(hip, monkeypatch, method):
    """At 4 queues the plan has no input stream: pinned host clouds handed over without waiting are copied on the frames' own
    ray-generation streams, 12 frames through 6 staging sets."""
    import torch
    ref = reference(hip, monkeypatch, method, 0.05)
    layer, integ = planned_for(hip, monkeypatch, 4, method, 0.05)
    host = [(T, torch.from_numpy(p).pin_memory(), torch.from_numpy(c).pin_memory()) for T, p, c in frames()]
    for T, xyz, rgba in host:
        integ.integrate_points_async(T, xyz.data_ptr(), rgba.data_ptr(), xyz.shape[0])
    integ.wait_inputs()
    integ.sync()
    same(layer, integ, ref)
