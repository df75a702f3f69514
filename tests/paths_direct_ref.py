"""srtTracePathsDirectDevice (include/srt_hip.h "Direct light sampling") stated through the entries of a user-land loop: per
bounce srtTraceRaysDevice with records, srtDirectLightDevice on them, srtScatterRaysDevice -- and the drop rule and the
unwinding L = D_j + L * att_j in NumPy float32 (a multiply, then an add).  What the tests of the one-kernel entry compare it
to.  The queries have no mask: an entry that has ended gets an empty interval (tMax = 0), so that it misses, scatters
nothing and keeps its state, as pathloop's unfused loop does it."""
import numpy as np

import direct_scenes as DS

F = np.float32


def loop(ctx, abi, sb, rays, rng0, max_bounce, background, traversal, spheres=None, cases=None):
    """rays (n, 9) float32, rng0 (n,) int64 on the host; sb: the uploaded scene's builder, spheres: its SPHERE_DTYPE records
    after an update (None: as built).  Returns paths_ref.loop's dict.  cases: a dict that receives how many entries met each
    case of the drop rule and of the term."""
    import torch
    rays = np.ascontiguousarray(rays, F).reshape(-1, 9)
    n = len(rays)
    table = {prim: (c, r, moving) for prim, c, r, moving in DS.light_table(sb, spheres)}
    K = len(table)
    pbr = np.zeros(len(sb.materials) + 1, bool)
    pbr[DS.pbr_materials(sb)] = True
    steps = np.zeros(n, np.int16)
    status = np.full(n, abi.SRT_PATH_SCATTERED, np.int16)
    terminal = np.zeros((n, 3), F)
    levels = []  # per step: (who scattered, attenuation, direct term)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_rng = torch.from_numpy(np.ascontiguousarray(rng0, np.int64).copy()).cuda()
    on = np.ones(n, bool)
    sampled_before = np.zeros(n, bool)
    count = {"dropped": 0, "kept: camera ray or not after pbr": 0, "kept: moving": 0, "kept: inside": 0, "kept: not in S": 0,
             "term > 0": 0, "term 0: shadowed or below the horizon": 0, "nothing sampled": 0}
    for _ in range(max_bounce if n else 0):
        if not on.any():
            break
        d_rays[:, 8].masked_fill_(torch.from_numpy(~on).cuda(), 0.0)
        origin = d_rays[:, 0:3].cpu().numpy()
        _, records = ctx.trace_device(d_rays, traversal, records=True)
        direct = ctx.direct_light_device(d_rays, records, d_rng, traversal)  # ahead of the scatter: the states before its draws
        out, _ = ctx.scatter_device(d_rays, records, d_rng, rays_out=d_rays)
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(abi.PATH_OUT_DTYPE).reshape(-1)
        d = direct.cpu().numpy().view(abi.DIRECT_OUT_DTYPE).reshape(-1)
        rec = records.cpu().numpy().view(abi.HIT_DTYPE).reshape(-1)
        steps[on] += 1
        status[on] = o["status"][on]
        terminal[on & (o["status"] == abi.SRT_PATH_MISS)] = np.asarray(background, F)
        ended = on & (o["status"] == abi.SRT_PATH_ENDED)
        emitted = o["emitted"].copy()
        for i in np.flatnonzero(ended):  # the drop rule
            prim = int(o["prim"][i])
            if prim not in table:
                count["kept: not in S"] += 1
                continue
            c, r, moving = table[prim]
            v = c - origin[i]
            outside = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > r * r
            if not sampled_before[i]:
                count["kept: camera ray or not after pbr"] += 1
            elif moving:
                count["kept: moving"] += 1
            elif not outside:
                count["kept: inside"] += 1
            else:
                count["dropped"] += 1
                emitted[i] = 0.0
        terminal[ended] = emitted[ended]
        hit_pbr = (rec["prim"] >= 0) & (rec["material"] >= 0) & (rec["material"] < len(sb.materials)) & pbr[np.clip(rec["material"], 0, len(sb.materials))]
        sampled = on & hit_pbr & (K > 0)
        assert (d["light"][~sampled] == -1).all() and not d["radiance"][~sampled].any()
        count["nothing sampled"] += int((sampled & (d["light"] < 0)).sum())
        count["term > 0"] += int((sampled & (d["radiance"] > 0).any(axis=1)).sum())
        count["term 0: shadowed or below the horizon"] += int((sampled & (d["light"] >= 0) & ~d["radiance"].any(axis=1)).sum())
        on = on & (o["status"] == abi.SRT_PATH_SCATTERED)
        assert (on[sampled]).all()  # pbr always scatters
        levels.append((on, o["attenuation"].copy(), np.where(sampled[:, None], d["radiance"], F(0.0)).astype(F)))
        sampled_before = sampled
    radiance = terminal
    with np.errstate(all="ignore"):
        for went_on, attenuation, term in reversed(levels):  # L = D_j + L * attenuation_j, innermost first
            radiance[went_on] = term[went_on] + radiance[went_on] * attenuation[went_on]
    torch.cuda.synchronize()
    if cases is not None:
        for k, v in count.items():
            cases[k] = cases.get(k, 0) + v
    return {"radiance": radiance, "steps": steps, "status": status, "rng": d_rng.cpu().numpy()}
