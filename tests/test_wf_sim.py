"""The wave model of the path-pool kernel's inner loop (tools/wf_sim.py), no GPU: on 1 000 recorded rays of the headline
frame the baseline policy's node fill lies where the device measured it -- 32.6 lanes per visit in
profiles/r25/wf_profile_masterchief_change.txt, 33.0 in the model on 3 000 rays; the band is 30-36 -- and taking the head of
every walk out of the loop (--head, the tunable "wf_head") lowers the traversal instructions per ray."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def sim(oracle, dev):  # (the fixtures build the oracle and the library where they are missing)
    spec = importlib.util.spec_from_file_location("wf_sim", os.path.join(ROOT, "tools", "wf_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(sim):
    seqs, head = sim.masterchief_sequences(1000)
    return seqs, head


def _per_ray(st):
    return (st["node_instr"] + st["prim_instr"] + st["swap_instr"]) / st["rays"]


def test_baseline_node_fill(sim, recorded):
    seqs, _ = recorded
    assert len(seqs) == 1000
    steps = np.array([[(s == k).sum() for k in (sim.NODE, sim.SPHERE, sim.TRI)] for s in seqs]).mean(axis=0)
    assert 19.0 < steps[0] < 24.0 and 1.4 < steps[1] < 2.0, steps  # the replay of the issue: 21.7 visits, 1.7 sphere tests per ray
    st = sim.simulate(seqs)
    fill = st["node_lanes"] / st["node_runs"]
    print("baseline: %.2f instructions per ray, node fill %.1f lanes over %d visits" % (_per_ray(st), fill, st["node_runs"]))
    assert 30.0 <= fill <= 36.0, fill
    assert 900 < st["rays"] <= 1000


def test_head_lowers_instructions_per_ray(sim, recorded):
    seqs, head = recorded
    assert head == 2  # the headline's leading leaf holds two spheres
    base = sim.simulate(seqs)
    cut = sim.take_head(seqs, head)
    assert all(len(a) - len(b) in (1, 3) for a, b in zip(seqs, cut))
    with_head = sim.simulate(cut, head=True)
    print("instructions per ray: %.2f -> %.2f with the head" % (_per_ray(base), _per_ray(with_head)))
    assert with_head["swap_instr"] > base["swap_instr"] * 1.5  # the head is paid for in the swap step
    assert _per_ray(with_head) < _per_ray(base)
