"""A NumPy / Python-int mirror of the counter RNG (csrc/srt_path.h Pcg) for the path-step tests: mix64, the key of a
(seed, pixel, sample), the 64-bit LCG step with the XSH-RR output, `uniform` in float32 and the disk and sphere rejection
loops, so that a test can say which state a stream is in after a known sequence of draws.  tests/test_pathstep_abi.py pins
it to the oracle's generator."""
import numpy as np

F = np.float32
M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_key(seed, pixel, sample):
    """The state a render gives (pixel, sample) before its first draw (srtRngKey)."""
    return mix64(mix64(seed & M64) ^ (((pixel & 0xffffffff) << 32) | (sample & 0xffffffff)))


def as_int64(state):
    """A state as a torch / NumPy int64 holds it."""
    return state - (1 << 64) if state >= (1 << 63) else state


def from_int64(value):
    return int(value) & M64


class Pcg:
    def __init__(self, state):
        self.state = state & M64

    def bits(self):
        old = self.state
        self.state = (old * 6364136223846793005 + 1442695040888963407) & M64
        xs = (((old >> 18) ^ old) >> 27) & 0xffffffff
        rot = old >> 59
        return ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xffffffff

    def uniform(self):
        r = F(self.bits()) * F(2.3283064365386963e-10)  # float(u32), rounded to nearest even, times 2^-32
        return F(np.nextafter(F(1.0), F(0.0))) if r >= F(1.0) else r

    def uniform_range(self, lo, hi):
        return F(lo) + (F(hi) - F(lo)) * self.uniform()

    def in_unit_disk(self):
        """(x, y): y is drawn first (vec3.h:88-95)."""
        while True:
            y = self.uniform_range(-1.0, 1.0)
            x = self.uniform_range(-1.0, 1.0)
            if (x * x + y * y) + F(0.0) * F(0.0) >= F(1.0):
                continue
            return x, y

    def in_unit_sphere(self):
        """(x, y, z): drawn z, y, x (vec3.h:62-70 with g++'s argument order)."""
        while True:
            z = self.uniform_range(-1.0, 1.0)
            y = self.uniform_range(-1.0, 1.0)
            x = self.uniform_range(-1.0, 1.0)
            if (x * x + y * y) + z * z >= F(1.0):
                continue
            return x, y, z


def after_camera_ray(seed, pixel, sample):
    """The state after the draws of one camera ray: u, v, the lens disk, the time."""
    g = Pcg(rng_key(seed, pixel, sample))
    g.uniform()
    g.uniform()
    g.in_unit_disk()
    g.uniform()
    return g.state
