"""Direct light sampling estimates the SAME image (include/srt_hip.h "Direct light sampling", expectation), and pathloop's two
direct forms render the same bits.

Same expectation: tests/direct_scenes.expectation -- 16 x 12, a pbr ground, two pbr spheres, one small bright light outside
the view -- rendered with M = 64 seeds x N = 1024 spp, plain whole paths against direct whole paths, FAITHFUL.  The statistic is
the frame's mean luminance over finite pixels; |mean_direct - mean_plain| must be at most 4 x the combined standard error
computed from the two sets' own spreads.  tests/test_direct_expectation.py shows on the CPU oracle that this margin is below
5 % of the part of the mean the light contributes (3.11 % with the plain spread on both sides), so a lost or doubled direct
term cannot pass.

Measured on an MI355X (the figures are also printed before they are asserted): plain mean 0.04674, standard deviation across
the 64 frames 0.00157; direct mean 0.04711, standard deviation 0.00016; unlit 0.01100, lit part 0.03574; difference +0.00037
against a margin of 4 * sqrt(0.00157^2 / 64 + 0.00016^2 / 64) = 0.00079, which is 2.21 % of the lit part.  The variance
across seeds falls to about a hundredth (0.00016^2 against 0.00157^2)."""
import numpy as np
import pytest
import torch

import direct_scenes as DS
from test_gpu_pathstep import _bits, pathloop  # noqa: F401

pytestmark = pytest.mark.gpu


def _means(ctx, abi, pathloop, direct):  # noqa: F811
    out = []
    for seed in range(DS.EXPECT_SEEDS):
        image = pathloop.render(ctx, DS.expectation_params(abi, seed), whole=True, direct=direct)
        out.append(DS.mean_luminance(image.cpu().numpy()))
    return np.array(out)


def test_direct_and_plain_have_the_same_expectation(ctx, dev, abi, pathloop):  # noqa: F811
    ctx.set_camera(dev.make_camera(DS.expectation_camera_params(abi)))
    ctx.upload_scene(DS.expectation(abi, False))
    dark = DS.mean_luminance(pathloop.render(ctx, DS.expectation_params(abi, 0), whole=True).cpu().numpy())
    ctx.upload_scene(DS.expectation(abi, True))
    assert len(ctx.sampled_lights()) == 1
    plain, direct = _means(ctx, abi, pathloop, False), _means(ctx, abi, pathloop, True)
    M = DS.EXPECT_SEEDS
    margin = 4 * np.sqrt(plain.var(ddof=1) / M + direct.var(ddof=1) / M)
    lit_part = plain.mean() - dark
    print("plain %.5f +- %.5f, direct %.5f +- %.5f (standard deviation across %d frames), unlit %.5f; difference %.5f, margin %.5f = %.2f %% of "
          "the lit part" % (plain.mean(), plain.std(ddof=1), direct.mean(), direct.std(ddof=1), M, dark, direct.mean() - plain.mean(), margin,
                            100 * margin / lit_part))
    assert margin < 0.05 * lit_part
    assert abs(direct.mean() - plain.mean()) <= margin, (direct.mean(), plain.mean(), margin)
    assert direct.var(ddof=1) < plain.var(ddof=1)


def _same_image(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(nan, np.isnan(got)), what
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


def test_direct_frame_is_the_render_where_nothing_is_sampled(ctx, abi, camera):
    """K = 0: srtRenderDirectImage equals srtRenderImage (sppChunks = 1, FAITHFUL) in every byte, whatever the batch."""
    ctx.upload_scene(DS.lit(abi, 0))
    ctx.set_camera(camera)
    assert len(ctx.sampled_lights()) == 0
    p = abi.default_render_params(24, 16, 5, 4, seed=7, spp_chunks=1)
    want_acc, want_rgba = ctx.render_image(p)
    assert (want_acc[..., 3] == 5).all() and len(np.unique(want_rgba)) > 20
    for batch in (2, 0, 5, 1):
        acc, rgba = ctx.render_direct_image(p, samples_per_batch=batch)
        _same_image(acc, want_acc, batch)
        assert rgba.tobytes() == want_rgba.tobytes(), batch
    acc, none = ctx.render_direct_image(p, 2, want_rgba=False)
    assert none is None and acc.tobytes() == ctx.render_direct_image(p, 2)[0].tobytes()
    with pytest.raises(Exception, match="negative"):
        ctx.render_direct_image(p, samples_per_batch=-1)


def test_pathloops_two_direct_forms_render_the_direct_frame(ctx, abi, camera, pathloop):  # noqa: F811
    sb = DS.lights(abi)
    ctx.upload_scene(sb)
    ctx.set_camera(camera)
    for traversal in (abi.SRT_TRAVERSE_FAITHFUL, abi.SRT_TRAVERSE_CLOSEST):
        p = abi.default_render_params(24, 16, 5, 4, seed=7, traversal=traversal)
        frame, frame_rgba = ctx.render_direct_image(p, samples_per_batch=2)
        assert frame.tobytes() == ctx.render_direct_image(p, samples_per_batch=0)[0].tobytes()  # the batch does not matter
        whole = pathloop.render(ctx, p, traversal=traversal, whole=True, direct=True, samples_per_batch=2)
        loop = pathloop.render(ctx, p, traversal=traversal, fused=False, direct=pathloop.direct_tables(ctx, sb), samples_per_batch=2)
        plain = pathloop.render(ctx, p, traversal=traversal, whole=True)
        torch.cuda.synchronize()
        _same_image(whole.cpu().numpy(), frame, (traversal, "whole"))
        _same_image(loop.cpu().numpy(), frame, (traversal, "loop"))
        assert frame.tobytes() != plain.cpu().numpy().tobytes()
        # the 8-bit form: the adaptive entries' quantisation of the sums (csrc/srt_device.h srtQuantise8), in NumPy float32
        mean = frame[..., :3] * (np.float32(1.0) / frame[..., 3:4])
        with np.errstate(all="ignore"):
            g = np.sqrt(mean)
            q = np.float32(256.0) * np.where(g < 0, np.float32(0), np.where(g > np.float32(0.999), np.float32(0.999), g)).astype(np.float32)
        want = np.where(np.isnan(q), 0, q).astype(np.uint8)
        assert np.array_equal(frame_rgba[..., :3], want) and (frame_rgba[..., 3] == 255).all()
    p = abi.default_render_params(24, 16, 5, 4, seed=7)
    with pytest.raises(ValueError, match="direct_tables"):
        pathloop.render(ctx, p, fused=False, direct=True)
    with pytest.raises(ValueError, match="unfused"):
        pathloop.render(ctx, p, fused=True, direct=pathloop.direct_tables(ctx, sb))
