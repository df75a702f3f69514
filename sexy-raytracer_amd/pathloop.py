"""The library's path tracer as a user-land loop over its device path steps (include/srt_hip.h "Path steps on device
buffers"): camera rays, then one step per bounce, then the unwinding, all on torch tensors that never leave the GPU.

With FAITHFUL steps render() reproduces Context.render_image's accumulation buffer bit for bit (sppChunks = 1); it is the
worked example for integrators of one's own (ambient occlusion with materials, direct-light passes, path-length AOVs):
everything between two steps is an ordinary torch op on `out`, `rays` and `active`.

Plumbing only: no arithmetic of the hot path lives here beyond the loop's stated multiply, add and running sum."""
from . import abi

_DEAD = -2  # a status no step writes: an entry that was not active in this step


def direct_tables(ctx, scene_builder, spheres=None, device=None):
    """What the unfused direct-light loop needs of the uploaded scene beside the library's calls, for its drop rule: (lights,
    prims, pbr) -- lights float32 (k, 4) on the GPU, {centre, radius} of the sampled lights (Context.sampled_lights) that do
    not move, prims their prims[] indices as a host list of ints, and pbr, a bool tensor over the materials.  scene_builder: the SceneBuilder that was uploaded; spheres:
    abi.SPHERE_DTYPE records of its spheres as they are now (after update_spheres), or None."""
    import numpy as np
    import torch
    device = torch.device("cuda" if device is None else device)
    kinds = np.concatenate(scene_builder._prim_chunks)
    rows, prims = [], []
    for prim in ctx.sampled_lights().tolist():
        i = int(kinds[prim, 1])
        s = scene_builder.spheres[i]
        c0, c1, radius = (s.center0[:], s.center1[:], s.radius) if spheres is None else (spheres["center0"][i], spheres["center1"][i], spheres["radius"][i])
        if tuple(np.float32(c0)) == tuple(np.float32(c1)):
            rows.append([float(v) for v in c0] + [float(radius)])
            prims.append(int(prim))
    lights = torch.tensor(rows, dtype=torch.float32, device=device).reshape(-1, 4)
    pbr = torch.tensor([m.type == abi.SRT_MAT_PBR for m in scene_builder.materials], dtype=torch.bool, device=device)
    return lights, prims, pbr


def _sample_radiance_direct(ctx, rays, rng, max_bounce, background, traversal, stream, tables):
    """sample_radiance with direct light sampling as a user-land loop: per bounce trace_device(records=True), then
    direct_light_device on the states as they are BEFORE the scatter, then scatter_device; the drop rule and the unwinding
    L = D_j + L * att_j are torch ops.  The bits of Context.trace_paths_device(direct=True)."""
    import torch
    lights, light_prims, pbr = tables
    n = rays.shape[0]
    sampling = len(ctx.sampled_lights()) > 0
    bg = torch.tensor([float(c) for c in background], dtype=torch.float32, device=rays.device)
    terminal = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
    active = torch.ones((n,), dtype=torch.bool, device=rays.device)
    sampled_before = torch.zeros((n,), dtype=torch.bool, device=rays.device)
    steps = []  # per step: (attenuation, direct term, scattered)
    for _ in range(max_bounce):
        rays[:, 8].masked_fill_(~active, 0.0)  # the queries have no mask: a finished entry misses
        origin = rays[:, 0:3].clone()
        _, records = ctx.trace_device(rays, traversal, records=True, stream=stream)
        direct = ctx.direct_light_device(rays, records, rng, traversal, stream=stream)
        out, _ = ctx.scatter_device(rays, records, rng, rays_out=rays, stream=stream)
        status = torch.where(active, out[:, 3], torch.full_like(out[:, 3], _DEAD))
        colours = out.view(torch.float32)
        scattered = status == abi.SRT_PATH_SCATTERED
        ended = status == abi.SRT_PATH_ENDED
        # the drop rule: a bounced ray that ends on a light the step before could have chosen loses that light's emission
        drop = torch.zeros_like(ended)
        for k, prim in enumerate(light_prims):
            v = lights[k, 0:3] - origin
            far = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2] > lights[k, 3] * lights[k, 3]
            drop |= (out[:, 7] == prim) & far
        emitted = torch.where((drop & sampled_before)[:, None], torch.zeros_like(terminal), colours[:, 4:7])
        terminal = torch.where((status == abi.SRT_PATH_MISS)[:, None], bg, terminal)
        terminal = torch.where(ended[:, None], emitted, terminal)
        material = records[:, 17].to(torch.int64).clamp(0, pbr.shape[0] - 1)
        sampled_before = scattered & pbr[material] & sampling
        term = torch.where(sampled_before[:, None], direct.view(torch.float32)[:, 0:3], torch.zeros_like(terminal))
        steps.append((colours[:, 0:3], term, scattered))
        active = scattered
    radiance = terminal
    for attenuation, term, scattered in reversed(steps):
        radiance = torch.where(scattered[:, None], radiance * attenuation + term, radiance)
    return radiance


def sample_radiance(ctx, rays, rng, max_bounce, background, traversal=abi.SRT_TRAVERSE_FAITHFUL, fused=True, stream=None,
                    active_counts=None, compact=False, whole=False, sort=None, direct=False):
    """The radiance of one path per ray: at most max_bounce steps, then the unwinding.  rays (n, 9) float32 and rng (n,)
    int64 as Context.camera_rays_device returns them; both are overwritten.  fused: one path_step_device per bounce;
    otherwise trace_device(records=True) + scatter_device, which compute the same bytes through an 88-byte record per ray.
    active_counts: a list that receives, per bounce, the number of entries still on their way (a 0-dim tensor: reading it
    synchronises, so read it after the loop).  compact: every bounce after the first runs on the live entries alone,
    moved to the front by Context.compact_paths_device (_sample_radiance_compact below): the same bits.  whole: no loop
    at all -- one Context.trace_paths_device call carries every path from its ray to its radiance in one kernel (the same
    bits again; rays is then only read, and there are no per-bounce counts to report).  sort: None, or the cell bits per
    axis (1 .. abi.SRT_SORT_MAX_CELL_BITS) of Context.sort_paths_device, which then takes the place of
    compact_paths_device in the compacted loop: the live entries move to the front AND into the order of their origin's
    cell and their direction's octant, in the box of their origins -- the same bits once more; not together with whole.
    direct: direct light sampling (include/srt_hip.h "Direct light sampling") -- another estimator of the same image, so
    other bits.  With whole=True any true value: one Context.trace_paths_device(direct=True) call.  Otherwise the
    direct_tables() of the uploaded scene: the unfused loop of trace records -> direct_light_device -> scatter_device with
    the drop rule and the unwinding as torch ops (fused=False; no compaction, sort or counts), the whole form's bits.
    Returns (n, 3) float32."""
    import torch
    if whole:
        _check_whole(fused, compact, active_counts, sort)
        return ctx.trace_paths_device(rays, rng, max_bounce, background, traversal, stream=stream, direct=bool(direct)).view(torch.float32)[:, 0:3]
    if direct is not False and direct is not None:
        if fused or compact or sort is not None or active_counts is not None:
            raise ValueError("direct light sampling as a loop is the unfused one: fused=False, and no compact, sort or active_counts")
        if direct is True:
            raise ValueError("direct light sampling as a loop needs direct=direct_tables(ctx, scene_builder)")
        return _sample_radiance_direct(ctx, rays, rng, max_bounce, background, traversal, stream, direct)
    if sort is not None:
        return _sample_radiance_compact(ctx, rays, rng, max_bounce, background, traversal, fused, stream, active_counts, sort)
    if compact:
        return _sample_radiance_compact(ctx, rays, rng, max_bounce, background, traversal, fused, stream, active_counts)
    n = rays.shape[0]
    bg = torch.tensor([float(c) for c in background], dtype=torch.float32, device=rays.device)
    terminal = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)  # maxBounce steps all scattered: black
    active = torch.ones((n,), dtype=torch.uint8, device=rays.device)
    steps = []  # per step: (attenuation (n, 3), scattered (n,) bool)
    for _ in range(max_bounce):
        if active_counts is not None:
            active_counts.append(active.sum(dtype=torch.int64))
        if fused:
            out, _ = ctx.path_step_device(rays, rng, traversal, active=active, rays_out=rays, stream=stream)
        else:
            # the queries have no mask: a finished entry's ray is given an empty interval, so that its walk ends at the root
            rays[:, 8].masked_fill_(active == 0, 0.0)
            _, records = ctx.trace_device(rays, traversal, records=True, stream=stream)
            out, _ = ctx.scatter_device(rays, records, rng, rays_out=rays, stream=stream)
        status = torch.where(active != 0, out[:, 3], torch.full_like(out[:, 3], _DEAD))
        colours = out.view(torch.float32)
        scattered = status == abi.SRT_PATH_SCATTERED
        terminal = torch.where((status == abi.SRT_PATH_MISS)[:, None], bg, terminal)
        terminal = torch.where((status == abi.SRT_PATH_ENDED)[:, None], colours[:, 4:7], terminal)
        steps.append((colours[:, 0:3], scattered))
        active = scattered.to(torch.uint8)
    # emitted + newColor * attenuation with emitted = 0, innermost first (main.cpp:49-51): a multiply, then an add
    radiance = terminal
    for attenuation, scattered in reversed(steps):
        radiance = torch.where(scattered[:, None], radiance * attenuation + 0.0, radiance)
    return radiance


def _sample_radiance_compact(ctx, rays, rng, max_bounce, background, traversal, fused, stream, active_counts, sort=None):
    """sample_radiance with the live set compacted between bounces.  Step j runs on the m_j entries that scattered in
    every step before it (m_0 = n), dense at the front of ping-pong ray and state buffers; its SrtPathOut rows are kept at
    that length together with the slot list that says which of its rows the m_(j+1) survivors were.  The unwinding goes
    through those lists innermost first with the same separate multiply and add.  The number kept is read once per
    bounce (8 bytes, a synchronisation) to size the next step, and the loop stops when nobody is left.  sort: the cell bits
    of Context.sort_paths_device, which then moves and orders the survivors; the slot lists of a sort are as injective as
    those of a compaction, so the unwinding is the same."""
    import torch
    n = rays.shape[0]
    bg = torch.tensor([float(c) for c in background], dtype=torch.float32, device=rays.device)
    spare_rays, spare_rng = torch.empty_like(rays), torch.empty_like(rng)
    scratch_bytes = ctx.compact_scratch_bytes(n) if sort is None else ctx.sort_scratch_bytes(n)  # for n: for every m <= n
    scratch = torch.empty((max(scratch_bytes, 8),), dtype=torch.uint8, device=rays.device)
    steps = []  # per step: (out (m_j, 8) int32, slot (m_(j+1),) int32 or None behind the last step)
    m, live = n, torch.tensor(n, dtype=torch.int64, device=rays.device)
    for bounce in range(max_bounce):
        if active_counts is not None:
            active_counts.append(live if m else torch.zeros_like(live))
        if m == 0:
            continue
        step_rays, step_rng = rays[:m], rng[:m]
        if fused:
            out, _ = ctx.path_step_device(step_rays, step_rng, traversal, rays_out=step_rays, stream=stream)
        else:
            _, records = ctx.trace_device(step_rays, traversal, records=True, stream=stream)
            out, _ = ctx.scatter_device(step_rays, records, step_rng, rays_out=step_rays, stream=stream)
        if bounce + 1 == max_bounce:
            steps.append((out, None))
            break
        # every entry of this step was live: its status alone is the predicate
        if sort is None:
            _, _, slot, _, live = ctx.compact_paths_device(out=out, rays=step_rays, rng=step_rng, rays_out=spare_rays[:m],
                                                           rng_out=spare_rng[:m], scratch=scratch, stream=stream)
        else:
            _, _, slot, _, live = ctx.sort_paths_device(sort, out=out, rays=step_rays, rng=step_rng, rays_out=spare_rays[:m],
                                                        rng_out=spare_rng[:m], scratch=scratch, stream=stream)
        m = int(live)
        steps.append((out, slot[:m]))
        rays, spare_rays, rng, spare_rng = spare_rays, rays, spare_rng, rng
    # emitted + newColor * attenuation with emitted = 0, innermost first (main.cpp:49-51): a multiply, then an add
    inner = None  # the radiance of the entries of the step above
    for out, slot in reversed(steps):
        status, colours = out[:, 3], out.view(torch.float32)
        radiance = torch.zeros((out.shape[0], 3), dtype=torch.float32, device=out.device)
        radiance = torch.where((status == abi.SRT_PATH_MISS)[:, None], bg, radiance)
        radiance = torch.where((status == abi.SRT_PATH_ENDED)[:, None], colours[:, 4:7], radiance)
        if slot is None:  # maxBounce steps all scattered: black, through the last attenuation like every other
            radiance = torch.where((status == abi.SRT_PATH_SCATTERED)[:, None], radiance * colours[:, 0:3] + 0.0, radiance)
        elif slot.shape[0]:
            index = slot.to(torch.int64)
            radiance.index_copy_(0, index, inner * colours.index_select(0, index)[:, 0:3] + 0.0)
        inner = radiance
    return inner if inner is not None else torch.zeros((n, 3), dtype=torch.float32, device=rays.device)


def _check_whole(fused, compact, active_counts, sort=None):
    """whole=True has no bounces of its own to fuse, to compact or sort between or to count."""
    if not fused:
        raise ValueError("whole=True runs one kernel per batch: fused=False does not apply")
    if compact:
        raise ValueError("whole=True refills its waves itself: compact=True does not apply")
    if sort is not None:
        raise ValueError("whole=True refills its waves itself: sort does not apply")
    if active_counts is not None:
        raise ValueError("whole=True reads no count per bounce: active_counts does not apply")


def render(ctx, params, fused=True, traversal=abi.SRT_TRAVERSE_FAITHFUL, samples_per_batch=None, device=None, active_counts=None,
           compact=False, whole=False, sort=None, direct=False):
    """params.spp samples of every pixel from params.sampleFirst on, through the device path steps: the (H, W, 4) float32
    torch tensor of per-pixel radiance sums (the float running sum in sample-index order) with the sample count in w --
    Context.render_image's accumulation buffer.  samples_per_batch: how many sample indices of the whole frame go through
    the loop at once (default all; a batch holds about 8 * maxBounce + 25 words per entry: every step's SrtPathOut stays alive for the unwinding).  compact, sort: sample_radiance's.
    whole: a batch is one Context.trace_paths_device call (15 words per entry whatever maxBounce is) followed by the same
    running sum; not together with active_counts, compact, sort or fused=False.  direct: sample_radiance's -- True with
    whole=True, direct_tables(ctx, scene_builder) with fused=False; the two forms render the same bits, which are not
    Context.render_image's (another estimator of the same image).  Runs on torch's current stream."""
    import torch
    if whole:
        _check_whole(fused, compact, active_counts, sort)
    device = torch.device("cuda" if device is None else device)
    W, H, spp = params.imageWidth, params.imageHeight, params.spp
    pixels = W * H
    batch = spp if not samples_per_batch else max(1, min(int(samples_per_batch), spp))
    image = torch.zeros((pixels, 4), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        pixel = torch.arange(pixels, dtype=torch.int32, device=device)
        for first in range(0, spp, batch):
            count = min(batch, spp - first)
            # sample-major entries: the samples of one index are one contiguous slice of the batch
            pixel_sample = torch.stack((pixel.repeat(count),
                                        torch.arange(params.sampleFirst + first, params.sampleFirst + first + count, dtype=torch.int32,
                                                     device=device).repeat_interleave(pixels)), dim=1).contiguous()
            rays, rng = ctx.camera_rays_device(params, pixel_sample, stream=stream)
            radiance = sample_radiance(ctx, rays, rng, params.maxBounce, params.background, traversal, fused, stream, active_counts, compact,
                                       whole, sort, direct)
            for k in range(count):
                image[:, 0:3] += radiance[k * pixels:(k + 1) * pixels]
        image[:, 3] = float(spp)
    return image.view(H, W, 4)
