"""The design of the same-expectation test (tests/test_gpu_direct_expectation.py), checked on the CPU oracle with the PLAIN
estimator alone: with N = EXPECT_SPP samples per pixel in each of M = EXPECT_SEEDS frames, four combined standard errors of
the two sets' means stay below 5 % of the part of the frame's mean luminance that the light contributes -- so a direct term
that is lost or counted twice (a shift of that whole part, at the least of its directly lit share) cannot pass.  The margin
is derived from the sets' own spreads, not tuned; here the direct set's spread is taken to be the plain one's, which the GPU
test shows it stays below.

Measured (oracle, counter RNG, seeds 1000 .. 1063, 16 x 12 at 1024 spp): plain mean 0.04674, unlit mean 0.01100, standard
deviation across the frames 0.00157; margin 4 * sqrt(2 * 0.00157^2 / 64) = 0.00111 = 3.11 % of the lit part 0.03574.  (With
the light inside the view the pixels that see it carry the frame's mean and its spread: it hangs outside.)"""
import numpy as np

import direct_scenes as DS


def test_plain_renders_meet_the_margin(abi, oracle):
    cam = oracle.make_camera(DS.expectation_camera_params(abi))
    lit, unlit = oracle.OracleScene(DS.expectation(abi, True)), oracle.OracleScene(DS.expectation(abi, False))
    means = []
    for seed in range(DS.EXPECT_SEEDS):
        acc, _, _ = lit.render(cam, DS.expectation_params(abi, seed), oracle.RNG_COUNTER, threads=8, want_rgba=False, want_stats=False)
        assert np.isfinite(acc).all()
        means.append(DS.mean_luminance(acc))
    dark, _, _ = unlit.render(cam, DS.expectation_params(abi, 0), oracle.RNG_COUNTER, threads=8, want_rgba=False, want_stats=False)
    means = np.array(means)
    plain, spread = means.mean(), means.std(ddof=1)
    lit_part = plain - DS.mean_luminance(dark)
    margin = 4 * np.sqrt(2 * spread ** 2 / DS.EXPECT_SEEDS)
    print("plain mean %.5f, unlit mean %.5f, spread across frames %.5f, margin %.5f = %.2f %% of the lit part %.5f"
          % (plain, DS.mean_luminance(dark), spread, margin, 100 * margin / lit_part, lit_part))
    assert lit_part > 0.5 * plain, "the frame is lit by the light"
    assert margin < 0.05 * lit_part, (margin, lit_part)
