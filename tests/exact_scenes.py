"""Scenes whose shading makes no single-precision libm call, so that the render kernels and the CPU oracle perform the
same IEEE operations in the same order and a whole frame can be compared with no tolerance (tests/test_exact_scenes.py,
tests/test_gpu_exact_frames.py).  From shade() (csrc/srt_path.h):

  * metal: reflect, rejection-sampled fuzz -- +, *, /, sqrtf;
  * dielectric: sqrtf, and the reflectance's fifth power in double (the kernel writes the product out, the oracle calls
    the double pow);
  * a light with a solid colour, and the background: no arithmetic at all;
  * pbr with constant factors or solid-colour textures: ONE libm call, the DOUBLE exp2 of fresnelEpic narrowed to float.

A sphere's uv goes through acosf / atan2f, but nothing reads it where no image or checker is attached.

Tier "A" uses the first three only and must be exact unconditionally.  Tier "B" adds pbr (factors only, and a `solid`
albedo texture, on spheres and on triangles, so that all three material classes of the path pool occur); one of its pbr
materials has roughness 0, whose D term is 0 / 0 = NaN where the half vector meets the normal (rare at the
tests' sample counts, compared by position wherever it occurs).  Its only way to differ is the two double exp2 / pow
straddling a float rounding boundary.

The builders are plain functions of `abi` (and `srt` for the mesh), seeded; every result has passed assert_libm_free."""
import numpy as np

TIERS = ("A", "B")
METAL_FUZZ = (0.0, 0.05, 0.4, 1.0)
DIELECTRIC_IR = (1.5, 2.4)


def assert_libm_free(sb, tier):
    """Structural: every material of `sb` is of a kind the tier allows and every texture a material references is a solid
    colour; every primitive names one of these materials."""
    assert tier in TIERS
    abi = _abi(sb)
    assert len(sb.materials) > 0
    for k, m in enumerate(sb.materials):
        refs = {"albedoTex": m.albedoTex, "normalTex": m.normalTex, "metallicTex": m.metallicTex, "roughnessTex": m.roughnessTex}
        if m.type in (abi.SRT_MAT_METAL, abi.SRT_MAT_DIELECTRIC):
            assert all(t == -1 for t in refs.values()), (k, refs)
        elif m.type == abi.SRT_MAT_LIGHT:
            assert m.albedoTex >= 0 and all(refs[f] == -1 for f in ("normalTex", "metallicTex", "roughnessTex")), (k, refs)
        elif m.type == abi.SRT_MAT_PBR:
            assert tier == "B", "material %d: pbr (a double exp2) in a tier-A scene" % k
            # a normal map would go through the tangent frame, metallic / roughness maps are image lookups in every scene
            # the project has: only the albedo slot may hold a texture, and only a solid colour
            assert all(refs[f] == -1 for f in ("normalTex", "metallicTex", "roughnessTex")), (k, refs)
        else:
            raise AssertionError("material %d has unknown type %d" % (k, m.type))
        for f, t in refs.items():
            if t != -1:
                assert 0 <= t < len(sb.textures), (k, f, t)
                assert sb.textures[t].kind == abi.SRT_TEX_SOLID, "material %d: %s is texture %d of kind %d" % (k, f, t, sb.textures[t].kind)
    for tri in sb.triangles:
        assert ((tri["material"] >= 0) & (tri["material"] < len(sb.materials))).all()
    for s in sb.spheres:
        assert 0 <= s.material < len(sb.materials)
    return sb


def _abi(sb):
    import importlib
    return importlib.import_module(type(sb).__module__)


def material_kinds(sb):
    """The set of (type, has an albedo texture) over the materials that primitives use, split by primitive kind:
    {"sphere": {...}, "triangle": {...}}."""
    out = {"sphere": set(), "triangle": set()}
    for tri in sb.triangles:
        for k in np.unique(tri["material"]):
            out["triangle"].add((sb.materials[k].type, sb.materials[k].albedoTex >= 0))
    for s in sb.spheres:
        out["sphere"].add((sb.materials[s.material].type, sb.materials[s.material].albedoTex >= 0))
    return out


def palette(sb, rng, tier):
    """The tier's materials in a fixed order: the four metals, the two dielectrics, a light; tier B: then pbr with factors
    only (roughness 0 first: its NaN samples), pbr with a solid albedo texture twice."""
    mats = [sb.metal(tuple(rng.uniform(0.3, 1, 3)), fuzz) for fuzz in METAL_FUZZ]
    mats += [sb.dielectric(ir) for ir in DIELECTRIC_IR]
    mats.append(sb.light(tuple(rng.uniform(1, 20, 3))))
    if tier == "B":
        mats.append(sb.pbr(albedo=(0.8, 0.5, 0.3, 1.0), metalness=0.5, roughness=0.0))
        mats.append(sb.pbr(albedo=tuple(rng.uniform(0.2, 1, 4)), metalness=float(rng.uniform()), roughness=float(rng.uniform(0.05, 1))))
        mats.append(sb.pbr(albedo_tex=sb.solid(*rng.uniform(20, 240, 3)), metalness=float(rng.uniform()), roughness=float(rng.uniform(0.05, 1))))
        mats.append(sb.pbr(albedo_tex=sb.solid(*rng.uniform(20, 240, 3)), albedo=tuple(rng.uniform(0.2, 1, 4)), metalness=0.0, roughness=0.5))
    return mats


def random(abi, seed, tier, max_spheres=12):
    """tests/test_gpu_random_scenes.random_scene with the tier's materials: 1-60 triangles with its degenerate (zero area)
    and axis-aligned ones, tiny, huge and moving spheres, a ground, and its three world layouts (seed % 3: one tree; two trees and
    a bare primitive; a plain list).  Tier B: the triangles come in two groups, the first pbr with a solid albedo texture."""
    rng = np.random.default_rng([seed, TIERS.index(tier)])
    sb = abi.SceneBuilder()
    mats = palette(sb, rng, tier)
    n_tri = int(rng.integers(1, 60))
    pos = (rng.uniform(-3, 3, (n_tri * 3, 3)) + np.array([0, 3, -1])).astype(np.float32)
    for k in range(0, n_tri, 7):
        pos[3 * k + 2] = pos[3 * k + 1]                       # repeated vertex: zero area
    for k in range(3, n_tri, 11):
        pos[3 * k:3 * k + 3, int(rng.integers(0, 3))] = 1.25  # axis-aligned: flat box axis gets padded
    uv = rng.uniform(-0.2, 1.2, (n_tri * 3, 2)).astype(np.float32)
    idx = np.arange(n_tri * 3).reshape(-1, 3)
    cut = n_tri // 2 if tier == "B" else 0
    if cut:
        sb.add_triangles(pos, uv, idx[:cut], mats[-2])
    sb.add_triangles(pos, uv, idx[cut:], mats[int(rng.integers(0, len(mats)))])
    first_sphere = sb.num_prims
    for _ in range(int(rng.integers(1, max_spheres))):
        c = rng.uniform(-3, 3, 3) + np.array([0, 3, -1])
        r = float(rng.choice([0.0, 1e-3, 0.3, 0.8, 50.0], p=[0.05, 0.1, 0.5, 0.3, 0.05]))
        moving = rng.uniform() < 0.4
        sb.add_sphere(tuple(c), r, mats[int(rng.integers(0, len(mats)))],
                      center1=tuple(c + rng.uniform(-0.5, 0.5, 3)) if moving else None, time0=0.0, time1=1.0)
    # the ground: tier A a fuzzy metal; tier B the pbr with roughness 0, as main.cpp's ground is (its NaN samples)
    sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[7] if tier == "B" else mats[2])
    layout = seed % 3  # by the seed, not drawn: any three consecutive seeds cover the three layouts
    if layout == 0:
        sb.world_bvh(0, None, 0.0, 1.0)
    elif layout == 1:  # two roots + a bare primitive
        sb.world_bvh(0, first_sphere, 0.0, 1.0)
        sb.world_bvh(first_sphere, sb.num_prims - first_sphere - 1, 0.0, 1.0)
        sb.world_prim(sb.num_prims - 1)
    else:              # plain list
        for i in range(sb.num_prims):
            sb.world_prim(i)
    sb.layout = layout
    return assert_libm_free(sb, tier)


def bvh_nodes(n):
    """Nodes of the reference's tree over n primitives (bvh.h:55-95): spans of 1 and 2 are one node, larger ones split in
    halves."""
    return 1 if n <= 2 else 1 + bvh_nodes(n // 2) + bvh_nodes(n - n // 2)


def random_with_tree(abi, tier, first_seed=0, min_nodes=25):
    """(seed, scene): the first random(seed >= first_seed) whose world is ONE tree of at least min_nodes nodes -- what the
    ring tests need (a single root; more than the 24 nodes the forced hybrid form keeps resident)."""
    for seed in range(first_seed, first_seed + 64):
        sb = random(abi, seed, tier)
        if sb.layout == 0 and bvh_nodes(sb.num_prims) >= min_nodes:
            return seed, sb
    raise AssertionError("no single-tree scene among 64 seeds")


def room(abi, tier):
    """_mirror_room of tests/test_gpu_parity.py with its pbr and checker spheres replaced: the camera and a few spheres
    inside a closed fuzzy-metal sphere, lit by a small light, so nearly every path runs to maxBounce."""
    sb = abi.SceneBuilder()
    sb.add_sphere((0.0, 0.0, 0.0), 30.0, sb.metal((0.9, 0.85, 0.8), 0.4))
    if tier == "B":
        sb.add_sphere((0.0, 1.0, 0.0), 1.0, sb.pbr(albedo=(0.7, 0.5, 0.3, 1.0), roughness=0.6))
    else:
        sb.add_sphere((0.0, 1.0, 0.0), 1.0, sb.metal((0.7, 0.5, 0.3), 1.0))
    sb.add_sphere((-2.5, 1.5, -1.0), 1.2, sb.dielectric(1.5))
    sb.add_sphere((2.5, 1.2, -0.5), 0.9, sb.metal((0.6, 0.7, 0.8), 0.05))
    sb.add_sphere((0.0, 8.0, -3.0), 4.0, sb.light((6.0, 5.0, 4.0)))
    if tier == "B":
        sb.add_sphere((1.0, -0.5, 2.0), 0.4, sb.pbr(albedo_tex=sb.solid(50.0, 200.0, 120.0), metalness=0.3, roughness=0.0))
    else:
        sb.add_sphere((1.0, -0.5, 2.0), 0.4, sb.dielectric(2.4))
    sb.add_sphere((-1.0, 3.5, 1.5), 0.5, sb.metal((0.8, 0.8, 0.3), 0.0))
    sb.world_bvh(0, None, 0.0, 1.0)
    return assert_libm_free(sb, tier)


def mesh(srt, abi, tier):
    """srt.scenes.scene_masterchief() -- its 3046 primitives and 4043-node tree unchanged -- with every entry of
    sb.materials rewritten in place to the tier's materials; no image or checker stays
    referenced (the textures themselves stay in the scene, unused)."""
    sb = srt.scenes.scene_masterchief()
    rng = np.random.default_rng([77, TIERS.index(tier)])
    donor = abi.SceneBuilder()
    pal = palette(donor, rng, tier)
    base = len(sb.textures)
    for t in donor.textures:  # the palette's solid colours, appended behind the scene's own textures
        assert t.kind == abi.SRT_TEX_SOLID
        sb.textures.append(t)
    # scene_masterchief's materials: 0 and 1 the mesh's (2976 and 66 triangles), 2 the ground, 3 the light sphere, 4 the iron
    # sphere, 5 the metal sphere.  By palette() index -- tier A: fuzz 0.4, glass 1.5, fuzz 1 ground, light, glass 2.4, mirror;
    # tier B: pbr with a solid texture and a fuzzy metal on the triangles, the roughness-0 pbr ground, light, pbr factors, glass
    order = {"A": (2, 4, 3, 6, 5, 0), "B": (9, 1, 7, 6, 8, 4)}[tier]
    assert len(sb.materials) == len(order)
    for k in range(len(sb.materials)):
        src = donor.materials[pal[order[k]]]
        m = abi.SrtMaterialIn.from_buffer_copy(bytes(src))
        if m.albedoTex >= 0:
            m.albedoTex += base
        sb.materials[k] = m
    return assert_libm_free(sb, tier)
