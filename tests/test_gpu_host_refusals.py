"""The one alias check of the ...Device entries that write planes of the caller's (WrittenPlanesOk of the host layer), through
each of the four entries that use it: an output that is one of the frames and two identical outputs raise Flow2DError and leave
every plane as it was -- the refusal comes before anything is queued --, disjoint planes are accepted and written."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, FRAMES, CAPACITY = 32, 24, 3, 256
FILL = 0x33


def interpolate(flow, frames, written, p):
    flow.interpolate_frames_device(frames, [0.5], written, p)


def track(flow, frames, written, p):
    flow.track_points_device(frames, written[:FRAMES], written[FRAMES:], CAPACITY, p)


def stabilise(flow, frames, written, p):
    flow.stabilise_sequence_device(frames, written, p, reference_index=1)


def denoise(flow, frames, written, p):
    flow.denoise_sequence_device(frames, written, p)


# entry, planes written, width and height of a written plane
ENTRIES = {
    "interpolate_frames_device": (interpolate, FRAMES - 1, W, H),
    "track_points_device": (track, 2 * FRAMES, CAPACITY, 1),
    "stabilise_sequence_device": (stabilise, FRAMES, W, H),
    "denoise_sequence_device": (denoise, FRAMES, W, H),
}


@pytest.fixture()
def scene(flow2d, ctx):
    """Three textured frames on the device, an OpticalFlow of their size and the smallest run there is: two pyramid levels, one
    outer and one inner iteration."""
    rng = np.random.default_rng(7)
    texture = rng.uniform(0, 255, (H, W + FRAMES)).astype(np.float32)
    images = [texture[:, k:k + W].copy() for k in range(FRAMES)]
    frames = [ctx.plane(W, H, a) for a in images]
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    yield flow, frames, images, flow.params(2, 0.5, 1, 1, 35.0, 0.001, 0.001, 5, 0.0)
    flow.close()


def written_planes(ctx, entry):
    _, count, w, h = ENTRIES[entry]
    return [ctx.plane(w, h).fill_bytes(FILL) for _ in range(count)]


def untouched(ctx, frames, images, planes):
    ctx.synchronize()
    pattern = np.frombuffer(bytes([FILL] * 4), np.float32)[0]
    return all(np.array_equal(f.download(), a) for f, a in zip(frames, images)) and all((q.download() == pattern).all() for q in planes)


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_output_that_is_a_frame_is_refused(flow2d, ctx, scene, entry):
    flow, frames, images, p = scene
    planes = written_planes(ctx, entry)
    with pytest.raises(flow2d.Flow2DError):
        ENTRIES[entry][0](flow, [f.ptr for f in frames], [frames[1].ptr] + [q.ptr for q in planes[1:]], p)
    assert untouched(ctx, frames, images, planes)


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_identical_outputs_are_refused(flow2d, ctx, scene, entry):
    flow, frames, images, p = scene
    planes = written_planes(ctx, entry)
    with pytest.raises(flow2d.Flow2DError):
        ENTRIES[entry][0](flow, [f.ptr for f in frames], [planes[0].ptr, planes[0].ptr] + [q.ptr for q in planes[2:]], p)
    assert untouched(ctx, frames, images, planes)


@pytest.mark.parametrize("entry", ENTRIES)
def test_disjoint_planes_are_accepted(flow2d, ctx, scene, entry):
    flow, frames, images, p = scene
    planes = written_planes(ctx, entry)
    ENTRIES[entry][0](flow, [f.ptr for f in frames], [q.ptr for q in planes], p)
    ctx.synchronize()
    assert all(np.array_equal(f.download(), a) for f, a in zip(frames, images))  # frames are only read
    assert not untouched(ctx, frames, images, planes[:1])  # ... and the outputs written
