"""The host stage of srtUploadScene (csrc/srt_scene.cpp: validateScene, flattenScene) on the host, no GPU: the stand-alone
program examples/scene_probe.cpp runs the library's own two functions over serialised scene descriptions
(tests/scene_probe_io.py) and writes every member of the HostScene they fill.

  * BIT FOR BIT AGAINST THE PARENT.  tests/golden/flatten_scenes.json holds, for the scenes of tests/scene_host_cases.py,
    every member's element count and the SHA-256 of its bytes, every scalar, and the text of every refusal.  It was recorded
    with the srt_scene.cpp OF THE COMMIT BEFORE flattenScene WAS CUT INTO STAGES linked into this probe
    (`python tests/make_golden.py flatten <that commit>`; the file names the commit).
  * PROPERTIES that do not rest on the recording: the triangle reordering is a permutation that the primitive ids follow,
    every reference word addresses an existing node or primitive, the hybrid renumbering is a permutation, and the sizes of
    the walk sequence and the class table.
  * REFUSALS: one minimal scene per `return` of validateScene, the full text.  Of flattenScene's three refusals none is
    reached: more than 2^25 nodes (a gigabyte of node slots), more than 2^24 materials, more than 2 GiB of texels.
  * the same program under the address and undefined-behaviour sanitizers, as a second stand-alone binary, over every scene
    and refusal, with the plain binary's bytes."""
import json
import os

import numpy as np
import pytest

import scene_host_cases as cases
import scene_probe_io as io
from conftest import GOLD

GOLDEN = os.path.join(GOLD, "flatten_scenes.json")
SRT_REF_DONE = -(1 << 31)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def probe():
    return io.build("srt_scene_probe")


@pytest.fixture(scope="module")
def scenes(srt, dev):
    """{name: (builder, desc, options, draws)}: built once (the iron textures are a second of noise).  (dev: the sphere field
    is placed with the library's host generator; no GPU is touched.)"""
    out = {}
    for name, make in cases.SCENES.items():
        sb, options = make(srt)
        out[name] = (sb, sb.desc(), options, int(getattr(sb, "global_rng_draws", 0)))
    return out


@pytest.fixture(scope="module")
def refused(srt):
    return {name: make(srt) for name, make in cases.REFUSALS.items()}


@pytest.fixture(scope="module")
def flattened(srt, probe, scenes, tmp_path_factory):
    d = tmp_path_factory.mktemp("flatten")
    return {name: io.flatten(probe, d, desc, srt.abi, options, draws)[0] for name, (_, desc, options, draws) in scenes.items()}


def test_cases_are_the_recorded_ones(golden):
    assert list(golden["scenes"]) == list(cases.SCENES) and list(golden["refusals"]) == list(cases.REFUSALS)
    assert "parent" in golden["recorded_with"]


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_flattened_bit_for_bit(golden, flattened, name):
    got, want = io.digest(flattened[name]), golden["scenes"][name]
    assert list(got) == list(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_every_member_is_reached(flattened):
    """Each vector of HostScene is non-empty, and each scalar non-zero, in at least one scene."""
    names = [k for k in flattened["spheres"] if "[" not in k]
    assert len(names) == 33
    for k in names:
        assert any(m[k].count > 0 or (m[k].count < 0 and m[k].data != bytes(4)) for m in flattened.values()), k
    assert any(m["itemNodes[0]"].count > 0 for m in flattened.values())
    assert any(m["deviceBuilds[0].refs"].count > 0 for m in flattened.values() if "deviceBuilds[0].refs" in m)
    both = {(i32(m, "fastDivScene")[0], i32(m, "boxOrderedScene")[0]) for m in flattened.values()}
    assert {(1, 1), (1, 0), (0, 1)} <= both


def i32(members, name):
    return np.frombuffer(members[name].data, "<i4")


def _references_exist(refs, num_nodes, num_triangles, num_spheres):
    refs = refs[refs != SRT_REF_DONE]
    node, prim = refs[refs >= 0], ~refs[refs < 0]
    assert not (node & 31).any() and (node >> 5 < max(num_nodes, 1)).all()
    sphere = (prim & 1) == 1
    assert ((prim >> 1)[sphere] < num_spheres).all() and ((prim >> 1)[~sphere] < num_triangles).all()


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_properties(scenes, flattened, name):
    sb, desc, _, _ = scenes[name]
    m = flattened[name]
    nt, ns = desc.numTriangles, desc.numSpheres
    num_nodes = m["nodes"].count // 2
    # the reordering: a permutation, and the primitive ids follow it
    dev = i32(m, "triDevIndex")
    assert len(dev) in (0, nt)
    if len(dev):
        assert np.array_equal(np.sort(dev), np.arange(nt))
    else:
        dev = np.arange(nt)
    prims = np.asarray(sb._keep[2]).reshape(-1, 2)
    listed = np.full(nt, -1, np.int64)
    tri = prims[:, 0] == 0
    listed[prims[tri, 1]] = np.nonzero(tri)[0]
    assert np.array_equal(i32(m, "triPrimId")[dev], listed)
    # references
    node_refs = np.frombuffer(m["nodes"].data, "<i4").reshape(-1, 4)[:, 3]
    _references_exist(node_refs, num_nodes, nt, ns)
    _references_exist(i32(m, "world"), num_nodes, nt, ns)
    assert m["world"].count == desc.numWorld
    for k in m:
        if k.endswith(".refs"):
            refs = i32(m, k)
            assert (refs < 0).all()
            _references_exist(refs, num_nodes, nt, ns)
    # the hybrid renumbering, the walk sequence, the class table
    if m["nodesWf"].count:
        assert np.array_equal(np.sort(i32(m, "wfIndex")), np.arange(num_nodes))
    else:
        assert m["wfIndex"].count == 0
    if m["walkSeq"].count:
        assert m["walkSeq"].count == 3 * i32(m, "numWalk")[0] + m["world"].count
    assert m["primClass"].count == 2 * max(nt, ns) + 2


@pytest.mark.parametrize("name", list(cases.REFUSALS))
def test_refusals(srt, golden, probe, refused, tmp_path, name):
    _, desc, carried = refused[name]
    text = golden["refusals"][name]
    assert text
    assert io.validate(probe, tmp_path, desc, srt.abi, carried) == text
    assert io.digest(io.flatten(probe, tmp_path, desc, srt.abi, carried=carried)[0]) == {"error": text}


def test_valid_scenes_validate_empty(srt, probe, scenes, tmp_path):
    for name in ("spheres", "mixed_world", "prebuilt"):
        assert io.validate(probe, tmp_path, scenes[name][1], srt.abi) == "", name


def test_refusal_texts_are_distinct_returns(golden):
    """21 cases over validateScene's 21 `return`s of a message; the two parents-of-a-node returns share their text."""
    texts = list(golden["refusals"].values())
    assert len(texts) == 21 and len(set(texts)) == 20


def test_probe_under_sanitizers(srt, scenes, refused, flattened, tmp_path):
    """validateScene and flattenScene under -fsanitize=address,undefined: a second stand-alone binary over every scene and
    every refusal, with the plain binary's bytes."""
    exe = io.build("srt_scene_probe_san")
    plain = io.build("srt_scene_probe")
    # (a stand-alone binary with the sanitizers' runtime linked in: the environment is inherited, plus their options)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name, (_, desc, options, draws) in scenes.items():
        assert io.flatten(exe, tmp_path, desc, srt.abi, options, draws, env=env)[0] == flattened[name], name
    for name, (_, desc, carried) in refused.items():
        want = io.flatten(plain, tmp_path, desc, srt.abi, carried=carried)[0]
        assert list(want) == ["error"]
        assert io.flatten(exe, tmp_path, desc, srt.abi, carried=carried, env=env)[0] == want, name
        assert io.validate(exe, tmp_path, desc, srt.abi, carried, env=env) == want["error"].data.decode(), name
