"""The scenes and the refused scenes of tests/test_scene_host.py (tests/make_golden.py records the same ones): small scenes
that between them reach every stage and branch of csrc/srt_scene.cpp flattenScene, and one minimal scene per refusal of
validateScene.

    SCENES    {name: function(srt) -> (SceneBuilder, options)}, options = (wf_hybrid, wf_resident_max, fast_div)
    REFUSALS  {name: function(srt) -> (SceneBuilder, desc, carried)}: the builder's desc(), damaged in one place; carried
              = {array: the elements the file holds} where that is not the count

Sizes: the whole-tree form of the path-pool kernel takes 4536 nodes (`srt_plan_probe limits`: whole_tree_max_nodes); the
reference-order build makes between n - 1 and 4n/3 nodes of n primitives, so 5001 primitives are above it and 301 below."""
import ctypes as C

import numpy as np

from scene_probe_io import DEFAULT_OPTIONS

SOUP_SMALL, SOUP_LARGE = 300, 5000
RESIDENT_CAP = 24  # wf_resident_max as conftest.py's "hybrid" node path sets it


def _image(rng, h, w, bpp):
    return rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)


def shading_records(srt):
    """One sphere per branch of the shading records: the five emit-texture forms of a light, the two checker albedos, a metal
    whose fuzz is clamped at upload, a dielectric; and a plain pbr with every slot an image (one of them 1 bpp)."""
    abi, rng = srt.abi, np.random.default_rng(11)
    sb = abi.SceneBuilder()
    solid = sb.solid(10.0, 20.0, 30.0)
    rgb, grey, failed = sb.image(_image(rng, 3, 5, 3), 3), sb.image(_image(rng, 2, 3, 1), 1), sb.image(None, 3)
    sb.textures.append(abi.SrtTextureIn(kind=abi.SRT_TEX_CHECKER, even=rgb, odd=solid))
    mixed = len(sb.textures) - 1
    mats = [sb.light((250.0, 220.0, 110.0)), sb.light(emit_tex=rgb), sb.light(emit_tex=grey), sb.light(emit_tex=failed),
            sb.light(emit_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))),
            sb.pbr(albedo_tex=sb.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)), roughness=0.5), sb.pbr(albedo_tex=mixed, roughness=0.5)]
    fuzzy = abi.SrtMaterialIn(type=abi.SRT_MAT_METAL, albedoTex=-1, normalTex=-1, metallicTex=-1, roughnessTex=-1, fuzz=1.5)
    fuzzy.albedo[:] = (0.7, 0.6, 0.5, 1.0)
    sb.materials.append(fuzzy)
    mats += [len(sb.materials) - 1, sb.dielectric(1.5),
             sb.pbr(albedo_tex=rgb, normal_tex=sb.image(_image(rng, 4, 4, 3), 3), metallic_tex=grey, roughness_tex=failed)]
    for i, m in enumerate(mats):
        sb.add_sphere((2.5 * (i % 4), 1.0 + 2.5 * (i // 4), 0.0), 1.0, m)
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def mixed_world(srt):
    """A device-built item over the first triangles, a host-built tree over the others (the triangle reordering puts ITS
    triangles first, so the device-built item's references go through it), a moving sphere under the PLOC builder, and a bare
    primitive."""
    abi = srt.abi
    sb = srt.scenes.scene_soup(40, seed=3, with_ground=False)
    sb.world = []
    moving = sb.add_sphere((0.0, 1.0, 0.0), 0.5, sb.dielectric(1.5), center1=(0.0, 2.0, 0.0), time0=0.0, time1=1.0)
    sb.add_sphere((3.0, 1.0, 0.0), 1.0, sb.metal((0.7, 0.6, 0.5), 0.0))
    bare = sb.add_sphere((0.0, -1000.0, 0.0), 1000.0, sb.pbr(roughness=0.5))
    sb.world_bvh(0, 15, 0.0, 1.0, builder=abi.SRT_BUILDER_LBVH)
    sb.world_bvh(15, 25, 0.0, 1.0)
    sb.world_bvh(moving, 2, 0.25, 0.75, builder=abi.SRT_BUILDER_PLOC)
    sb.world_prim(bare)
    return sb


def _three_spheres(srt, nodes=None, radius=1.0):
    """Three spheres in a row; nodes: the (left, right) pairs of a caller-built tree over them, or None for a tree to build.
    (Of radius -1 each has the box min = centre + 1, max = centre - 1, and no union of them is ordered in y.)"""
    sb = srt.abi.SceneBuilder()
    for x in (-3.0, 0.0, 3.0):
        sb.add_sphere((x, 1.0, 0.0), radius, sb.dielectric(1.5))
    if nodes is None:
        sb.world_bvh(0, None, 0.0, 1.0)
    if nodes is not None:
        a = np.zeros(len(nodes), srt.abi.NODE_DTYPE)
        a["bmin"], a["bmax"] = (-4.0, 0.0, -1.0), (4.0, 2.0, 1.0)
        a["left"], a["right"] = [n[0] for n in nodes], [n[1] for n in nodes]
        sb.world_prebuilt(a)
    return sb


def _far_sphere(srt):
    sb = srt.scenes.scene_spheres()
    sb.spheres[1].center0[:] = sb.spheres[1].center1[:] = (-3.0, 1.0, 3.0e9)  # fastDivOperand (srt_records.h) takes up to 2^30
    return sb


def _soup(srt, n, **kw):
    return srt.scenes.scene_soup(n, **kw)


SCENES = {
    "spheres": lambda srt: (srt.scenes.scene_spheres(), DEFAULT_OPTIONS),
    "sphere_field": lambda srt: (srt.scenes.scene_sphere_field(), DEFAULT_OPTIONS),  # generator draws before the build
    "iron": lambda srt: (srt.scenes.scene_iron(), DEFAULT_OPTIONS),
    "masterchief": lambda srt: (srt.scenes.scene_masterchief(), DEFAULT_OPTIONS),
    "soup_whole_tree": lambda srt: (_soup(srt, SOUP_SMALL), DEFAULT_OPTIONS),
    "soup_hybrid": lambda srt: (_soup(srt, SOUP_LARGE), DEFAULT_OPTIONS),
    "soup_no_hybrid": lambda srt: (_soup(srt, SOUP_LARGE), (0, 0, 1)),
    "soup_resident_cap": lambda srt: (_soup(srt, SOUP_LARGE), (1, RESIDENT_CAP, 1)),
    "soup_lbvh": lambda srt: (_soup(srt, SOUP_SMALL, builder=srt.abi.SRT_BUILDER_LBVH), DEFAULT_OPTIONS),
    "mixed_world": lambda srt: (mixed_world(srt), DEFAULT_OPTIONS),
    "prebuilt": lambda srt: (_three_spheres(srt, [(1, ~2), (~0, ~1)]), DEFAULT_OPTIONS),
    "negative_radius": lambda srt: (_three_spheres(srt, radius=-1.0), DEFAULT_OPTIONS),
    "beyond_fast_div": lambda srt: (_far_sphere(srt), DEFAULT_OPTIONS),
    "shading_records": lambda srt: (shading_records(srt), DEFAULT_OPTIONS),
}


# ------------------------------------------------------------------ refusals: one per `return` of validateScene, in its order
def _damaged(make, damage, carried=None):
    def case(srt):
        sb = make(srt)
        d = sb.desc()
        damage(srt.abi, sb, d)
        return sb, d, carried or {}
    return case


def _base(srt):
    """Triangles, spheres, an image, a checker, a light: something of every array."""
    sb = srt.scenes.scene_soup(4, with_ground=True)
    sb.add_sphere((0.0, 3.0, 0.0), 1.0, sb.light(emit_tex=sb.image(np.full((2, 2, 3), 200, np.uint8), 3)))
    sb.world = []
    sb.world_bvh(0, None, 0.0, 1.0)
    return sb


def _set(array, at, **fields):
    def damage(abi, sb, d):
        for k, v in fields.items():
            setattr(getattr(d, array)[at], k, v)
    return damage


def _desc(**fields):
    def damage(abi, sb, d):
        for k, v in fields.items():
            setattr(d, k, v)
    return damage


def _null_spheres(abi, sb, d):
    d.spheres = C.POINTER(abi.SrtSphereIn)()


def _tree(nodes):
    return lambda srt: _three_spheres(srt, nodes)


def _no_nodes(abi, sb, d):
    d.world[0].numNodes = 0


_keep = _desc()
CHECKER, IMAGE, LIGHT = 3, 4, 2  # _base's textures: soup solid, the ground's solid, solid, checker, the image; its materials: soup, ground, light
REFUSALS = {
    "negative_count": _damaged(_base, _desc(numSpheres=-1)),
    "null_array": _damaged(_base, _null_spheres),
    # (the count alone: the file carries the four triangles, and validateScene returns before it reads one)
    "too_many_primitives": _damaged(_base, _desc(numTriangles=0x40000000), {"triangles": 4}),
    "checker_child": _damaged(_base, _set("textures", CHECKER, even=CHECKER)),
    "image_dimensions": _damaged(_base, _set("textures", IMAGE, bpp=5)),
    "texels_out_of_range": _damaged(_base, _set("textures", IMAGE, texelOffset=1)),
    "texture_kind": _damaged(_base, _set("textures", 0, kind=7)),
    "material_type": _damaged(_base, _set("materials", 0, type=4)),
    "material_texture": _damaged(_base, _set("materials", 0, normalTex=99)),
    "light_without_texture": _damaged(_base, _set("materials", LIGHT, albedoTex=-1)),
    "triangle_material": _damaged(_base, _set("triangles", 2, material=3)),
    "sphere_material": _damaged(_base, _set("spheres", 1, material=-1)),
    "prim_index": _damaged(_base, _set("prims", 3, index=4)),
    "empty_world": _damaged(_base, _desc(numWorld=0)),
    "world_range": _damaged(_base, _set("world", 0, count=7)),
    "prebuilt_without_nodes": _damaged(_tree([(~0, ~1)]), _no_nodes),
    "prebuilt_child": _damaged(_tree([(1, ~2), (~0, ~3)]), _keep),
    "prebuilt_two_parents_left": _damaged(_tree([(1, 2), (2, ~0), (~1, ~2)]), _keep),
    "prebuilt_two_parents_right": _damaged(_tree([(1, 2), (~0, 2), (~1, ~2)]), _keep),
    "prebuilt_subtree_twice": _damaged(_tree([(1, 1), (~0, ~1)]), _keep),
    "prebuilt_unreachable": _damaged(_tree([(~0, ~1), (~1, ~2)]), _keep),
}
