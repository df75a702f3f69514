"""srtTracePathsDevice (include/srt_hip.h) stated through the entries that were there before it: the masked
srtPathStepDevice loop of the header's "the loop" paragraph, one launch per bounce with every entry's SrtPathOut read back,
and the unwinding in NumPy float32 (a multiply, then an add: two roundings, as the header says).  What the tests of the
one-kernel entry compare it to.  An entry's path depends on its own ray and state alone, so the loop over a ray set is also
the loop over every prefix of it."""
import numpy as np

F = np.float32


def loop(ctx, abi, rays, rng0, max_bounce, background, traversal):
    """rays (n, 9) float32 and rng0 (n,) int64 on the host.  Returns {"radiance": (n, 3) float32, "steps": (n,) int16,
    "status": (n,) int16, "rng": (n,) int64}: per entry what SrtPathRadiance and dRng[i] hold after the call."""
    import torch
    rays = np.ascontiguousarray(rays, F).reshape(-1, 9)
    n = len(rays)
    steps = np.zeros(n, np.int16)
    status = np.full(n, abi.SRT_PATH_SCATTERED, np.int16)  # also when no step runs
    terminal = np.zeros((n, 3), F)                         # INVALID, or every step scattered: black
    scattered_steps = []                                   # per step: (who scattered, the attenuations)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_rng = torch.from_numpy(np.ascontiguousarray(rng0, np.int64).copy()).cuda()
    on = np.ones(n, bool)
    for _ in range(max_bounce if n else 0):
        if not on.any():
            break
        out, _ = ctx.path_step_device(d_rays, d_rng, traversal, active=torch.from_numpy(on.astype(np.uint8)).cuda(), rays_out=d_rays)
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(abi.PATH_OUT_DTYPE).reshape(-1)
        steps[on] += 1
        status[on] = o["status"][on]
        terminal[on & (o["status"] == abi.SRT_PATH_MISS)] = np.asarray(background, F)
        ended = on & (o["status"] == abi.SRT_PATH_ENDED)
        terminal[ended] = o["emitted"][ended]
        on = on & (o["status"] == abi.SRT_PATH_SCATTERED)
        scattered_steps.append((on, o["attenuation"].copy()))
    radiance = terminal
    for went_on, attenuation in reversed(scattered_steps):  # L = 0.0f + L * attenuation, innermost first
        radiance[went_on] = F(0.0) + radiance[went_on] * attenuation[went_on]
    torch.cuda.synchronize()
    return {"radiance": radiance, "steps": steps, "status": status, "rng": d_rng.cpu().numpy()}


def prefix(ref, n):
    return {k: v[:n] for k, v in ref.items()}


def take(ref, index):
    return {k: v[index] for k, v in ref.items()}
