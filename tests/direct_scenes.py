"""Scenes for the direct-light tests (tests/test_gpu_direct.py) and what the tests' references need to know of a scene: its
sampled-light table as include/srt_hip.h "Direct light sampling" defines it, from the SceneBuilder alone."""
import numpy as np

F = np.float32


def sphere_of_prim(sb):
    """{prims[] index: index into sb.spheres}."""
    abi = _abi(sb)
    prims = np.concatenate(sb._prim_chunks) if sb._prim_chunks else np.zeros((0, 2), np.int32)
    return {p: int(i) for p, (t, i) in enumerate(prims) if t == abi.SRT_PRIM_SPHERE}


def _abi(sb):
    import importlib
    return importlib.import_module(type(sb).__module__)


def light_table(sb, spheres=None):
    """The sampled lights in prims[] order: [(prim, centre (3,) float32, radius float32, moving)].  spheres: SPHERE_DTYPE
    records that replace sb.spheres' geometry (after an update), or None."""
    abi = _abi(sb)
    out = []
    for prim, i in sorted(sphere_of_prim(sb).items()):
        s = sb.spheres[i]
        m = sb.materials[s.material]
        if m.type != abi.SRT_MAT_LIGHT:
            continue
        t = sb.textures[m.albedoTex]
        if not (t.kind == abi.SRT_TEX_SOLID or (t.kind == abi.SRT_TEX_IMAGE and t.width == 0)):
            continue
        if spheres is None:
            c0, c1, radius = np.array(s.center0[:], F), np.array(s.center1[:], F), F(s.radius)
        else:
            c0, c1, radius = spheres["center0"][i].astype(F), spheres["center1"][i].astype(F), F(spheres["radius"][i])
        out.append((prim, c0, radius, bool((c0 != c1).any())))
    return out


def light_colour(sb, prim):
    s = sb.spheres[sphere_of_prim(sb)[prim]]
    return np.array(sb.textures[sb.materials[s.material].albedoTex].color[:], F)


def sphere_records(sb):
    abi = _abi(sb)
    out = np.zeros(len(sb.spheres), abi.SPHERE_DTYPE)
    for i, s in enumerate(sb.spheres):
        out[i] = (tuple(s.center0[:]), tuple(s.center1[:]), s.time0, s.time1, s.radius, s.material)
    return out


def pbr_materials(sb, normal_mapped=None):
    """The indices of the pbr materials; normal_mapped: True / False keeps those with / without a normal map."""
    abi = _abi(sb)
    return [k for k, m in enumerate(sb.materials)
            if m.type == abi.SRT_MAT_PBR and (normal_mapped is None or (m.normalTex >= 0) == normal_mapped)]


def _furniture(sb):
    """pbr ground and spheres (factors, a solid albedo texture, a roughness-0 one), a metal and a glass sphere."""
    ground = sb.pbr(albedo=(0.6, 0.6, 0.55, 1.0), metalness=0.0, roughness=0.8)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, ground)
    sb.add_sphere((0.0, 1.0, 0.0), 1.0, sb.pbr(albedo=(0.7, 0.5, 0.3, 1.0), metalness=0.2, roughness=0.6))
    sb.add_sphere((-2.5, 1.2, -1.0), 1.2, sb.pbr(albedo_tex=sb.solid(50.0, 200.0, 120.0), metalness=0.6, roughness=0.3))
    sb.add_sphere((2.4, 0.9, 0.8), 0.9, sb.metal((0.8, 0.8, 0.9), 0.1))
    sb.add_sphere((0.8, 0.5, 2.2), 0.5, sb.dielectric(1.5))
    sb.add_sphere((-1.0, 0.4, 2.0), 0.4, sb.pbr(albedo=(0.8, 0.5, 0.3, 1.0), metalness=0.5, roughness=0.0))


STATIC_LIGHTS = (((0.0, 6.0, 1.0), 1.0, (25.0, 22.0, 11.0)), ((-5.0, 3.0, 2.0), 0.5, (4.0, 30.0, 8.0)), ((4.0, 2.5, -2.0), 0.7, (9.0, 3.0, 28.0)))


def lit(abi, k, builder=None):
    """The furniture under k of the three static solid-colour lights (K = k), one tree."""
    sb = abi.SceneBuilder()
    _furniture(sb)
    for centre, radius, colour in STATIC_LIGHTS[:k]:
        sb.add_sphere(centre, radius, sb.light(colour))
    sb.world_bvh(0, None, 0.0, 1.0, **({} if builder is None else {"builder": builder}))
    return sb


def lights(abi):
    """Three static solid lights; a moving light and a checker-emitting light, neither sampled; a metal triangle between the
    furniture and the first light (shadows); and, as a second world item beside the tree, a solid light of radius 30 that
    encloses everything: from inside d2 <= r^2, so choosing it samples nothing and its emission is kept.  K = 5: the three,
    the moving one, the enclosing one."""
    sb = abi.SceneBuilder()
    _furniture(sb)
    for centre, radius, colour in STATIC_LIGHTS:
        sb.add_sphere(centre, radius, sb.light(colour))
    sb.add_sphere((3.0, 4.0, 3.0), 0.6, sb.light((12.0, 12.0, 2.0)), center1=(3.5, 4.5, 3.0), time0=0.0, time1=1.0)
    sb.add_sphere((-3.0, 4.0, -3.0), 0.8, sb.light(emit_tex=sb.checker((0.05, 0.02, 0.01), (0.01, 0.04, 0.06))))
    pos = np.array([[-1.5, 3.5, 0.0], [1.5, 3.5, 0.0], [0.0, 3.5, 2.5]], F)
    sb.add_triangles(pos, np.zeros((3, 2), F), np.array([[0, 1, 2]]), sb.metal((0.9, 0.9, 0.9), 0.0))
    inner = sb.num_prims
    enclosing = sb.add_sphere((0.0, 0.0, 0.0), 30.0, sb.light((0.3, 0.35, 0.5)))
    sb.world_bvh(0, inner, 0.0, 1.0)
    sb.world_prim(enclosing)
    sb.enclosing, sb.moving_light, sb.checker_light = enclosing, inner - 3, inner - 2
    return sb


# ---- the same-expectation test (tests/test_gpu_direct_expectation.py, tests/test_direct_expectation.py)
EXPECT_W, EXPECT_H, EXPECT_BOUNCES = 16, 12, 4
EXPECT_SPP, EXPECT_SEEDS = 1024, 64  # N samples per pixel in each of M frames
EXPECT_BACKGROUND = (0.02, 0.02, 0.03)  # a dim sky: the frame is lit by the light


def expectation(abi, lit=True):
    """A pbr ground, two pbr spheres (no roughness 0: every pixel stays finite) and one small bright light above and in front
    of them, outside the camera's view: no pixel sees it directly, so the frame's light is what the bounces find.
    lit=False: the same light with its emission set to 0."""
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(albedo=(0.7, 0.7, 0.65, 1.0), metalness=0.0, roughness=0.7))
    sb.add_sphere((-1.3, 1.0, 0.0), 1.0, sb.pbr(albedo=(0.8, 0.4, 0.3, 1.0), metalness=0.1, roughness=0.5))
    sb.add_sphere((1.4, 0.8, 0.6), 0.8, sb.pbr(albedo=(0.3, 0.6, 0.8, 1.0), metalness=0.7, roughness=0.35))
    sb.add_sphere((0.5, 5.0, 3.0), 0.8, sb.light((60.0, 55.0, 40.0) if lit else (0.0, 0.0, 0.0)))
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def expectation_camera_params(abi):
    c = abi.default_camera_params(EXPECT_W / float(EXPECT_H))
    c.eye[:] = (0.0, 2.2, 6.5)
    c.lookAt[:] = (0.0, 1.0, 0.0)
    c.vfovDegrees, c.aperture, c.time0, c.time1 = 45.0, 0.0, 0.0, 0.0
    return c


def expectation_params(abi, seed, spp=EXPECT_SPP):
    return abi.default_render_params(EXPECT_W, EXPECT_H, spp, EXPECT_BOUNCES, seed=1000 + seed, background=EXPECT_BACKGROUND)


def mean_luminance(accum):
    """The frame's mean luminance over its finite pixels, from an accumulation buffer (H, W, 4): rgb sums, w the count."""
    a = np.asarray(accum, np.float64)
    rgb = a[..., :3] / a[..., 3:4]
    ok = np.isfinite(rgb).all(axis=-1)
    return float((rgb[ok] @ np.array([0.2126, 0.7152, 0.0722])).mean())


def rays_at(n, seed=3, inside=30.0):
    """n rays (n, 9) float32 from points around the furniture towards it, time in [0, 1), tMin 0.001, tMax inf."""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(6, 12, (n, 1))
    o[:, 1] = np.abs(o[:, 1]) + 0.5
    target = rng.uniform(-3, 3, (n, 3)) * np.array([1.0, 0.3, 1.0]) + np.array([0.0, 0.5, 0.0])
    rays = np.zeros((n, 9), F)
    rays[:, 0:3] = o
    rays[:, 3:6] = target - o
    rays[:, 6] = rng.uniform(0, 1, n)
    rays[:, 7] = 0.001
    rays[:, 8] = np.inf
    return rays
