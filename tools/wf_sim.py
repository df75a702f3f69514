#!/usr/bin/env python3
"""A model of one wave's inner loop in the path-pool kernel's whole-tree form (csrc/srt_wavefront.hip), for pricing a
scheduling idea before it gets device time.  No GPU: recorded rays of the headline frame are replayed on the CPU.

    python tools/wf_sim.py [--rays N] [--head] [--prim-min K] [--swap-min K] [--keep-eighths K] [--prim-again-min K]

What it does: records camera and bounce rays of the 720p masterchief frame with the CPU oracle, builds the regrouped tree
and its walk sequence through the library's host hooks (the replay helpers of tests/test_regroup_host.py and
tests/regroup_elide.py), turns every ray into its STEP SEQUENCE -- node visits, sphere tests, triangle tests, in the
walk's order -- and feeds the rays to one wave of 64 lanes that schedules as the kernel's loop does:

  * a node burst is SRT_NODE_UNROLL visits at a time, up to `node_burst` of them, and goes on while at least
    lanes-at-nodes x keep_eighths / 8 lanes are still at nodes;
  * a primitive step runs when `prim_min` lanes stand on a primitive (or none stands on a node): two rounds, the second
    only with `prim_again_min` lanes on a primitive again; a node burst follows it in the same trip with `fuse_min` lanes;
  * the rings are looked at when `swap_min` lanes are free, or every fourth trip; a swap refills every free lane (the
    READY ring never runs dry) and runs when it moves `swap_min` contexts -- finished walks out plus new rays in, as the
    kernel counts them -- or when nothing is left to traverse.  The run ends when the recorded rays cannot fill a swap:
    what is modelled is the steady state, not a wave's drain.

Costs are static instruction counts read off the listing: 24 per node visit, 58 per sphere test, 70 per triangle test
(a round pays for each kind that has a lane), 10 per round, 160 per swap.  --head models the head of the walks (tunable
"wf_head"): the leading leaf's visit and its sphere tests leave every ray's sequence, and a swap that starts a ray pays 140
more.  Output: traversal instructions per ray, split by step, and the mean fill of each step.

Its limits, which is why its numbers are for ranking ideas and not for predicting time:
  * the oracle's final t stands in for the running `closest`: a walk here culls more than a real one does early on;
  * there are no serve steps (hit shading, restarts, item pulls), no ring waits and one wave instead of sixteen;
  * the costs are static counts, not issue cycles, and a step's latency is not modelled at all;
  * it priced prim_min 16 at -2.5 % of the traversal instructions where the device measured 2.8 ms of 660:
    it overstated that effect by a factor of about six."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

F = np.float32
DONE = -(1 << 31)
NODE, SPHERE, TRI = 0, 1, 2
COST = {"visit": 24, "sphere": 58, "tri": 70, "round": 10, "swap": 160, "head": 140}
NODE_UNROLL, NODE_BURST, FUSE_MIN = 4, 64, 32


def step_sequences(rg, src, links, entry, passes, sphere_of):
    """Every ray's walk through the sequence for the box verdicts `passes` (rays x records of the binary array), as a list
    of uint8 arrays of NODE / SPHERE / TRI codes.  sphere_of(ref) tells a primitive reference's kind."""
    refs = rg.view(np.int32)
    kinds = []
    for j, s in enumerate(src):
        l, r = int(refs[s, 3]), int(refs[s, 7])
        kinds.append(None if l >= 0 else [SPHERE if sphere_of(x) else TRI for x in ((l,) if l == r else (l, r))])
    out = []
    for ray in range(passes.shape[0]):
        steps, cur = [], int(entry)
        while cur != DONE:
            j = cur >> 5
            steps.append(NODE)
            ok = bool(passes[ray, src[j]])
            if kinds[j] is None:
                cur = int(links[j, 0]) if ok else int(links[j, 1])
            else:
                if ok:
                    steps += kinds[j]
                cur = int(links[j, 1])
        out.append(np.array(steps, np.uint8))
    return out


def head_length(rg, src, sphere_of):
    """How many primitive tests the head takes off a ray whose head box passes, or None where the walks have no head."""
    refs = rg.view(np.int32)
    l, r = int(refs[src[0], 3]), int(refs[src[0], 7])
    if l >= 0 or not (sphere_of(l) and sphere_of(r)):
        return None
    return 1 if l == r else 2


def take_head(seqs, prims):
    """The sequences without their head: the leading visit, and the `prims` tests behind it where the box passed."""
    out = []
    for s in seqs:
        k = 1 + (prims if len(s) > 1 and s[1] != NODE else 0)
        assert s[0] == NODE and (s[1:k] == SPHERE).all()
        out.append(s[k:])
    return out


def simulate(seqs, prim_min=12, swap_min=32, keep_eighths=4, prim_again_min=4, head=False):
    """One wave over the rays in order.  Returns a dict of instruction counts, executions and lanes per step kind."""
    nxt = 0
    lane_seq = [None] * 64
    lane_pos = np.zeros(64, np.int64)
    st = {k: 0 for k in ("node_instr", "prim_instr", "swap_instr", "node_runs", "node_lanes", "prim_runs", "prim_lanes", "swap_runs", "swap_lanes", "rays")}

    def state():
        cur = np.full(64, -1, np.int64)  # -1: free
        for i in range(64):
            s = lane_seq[i]
            if s is not None and lane_pos[i] < len(s):
                cur[i] = s[lane_pos[i]]
        return cur

    def prim_step():
        for rnd in range(2):
            cur = state()
            at = cur > NODE
            if rnd > 0 and at.sum() < prim_again_min:
                break
            st["prim_runs"] += 1
            st["prim_lanes"] += int(at.sum())
            st["prim_instr"] += COST["round"] + (COST["sphere"] if (cur == SPHERE).any() else 0) + (COST["tri"] if (cur == TRI).any() else 0)
            lane_pos[at] += 1
        return int((state() == NODE).sum())

    def node_burst(n_nodes):
        keep = (n_nodes * keep_eighths) >> 3
        budget = NODE_BURST
        while True:
            for _ in range(NODE_UNROLL):
                at = state() == NODE
                st["node_runs"] += 1
                st["node_lanes"] += int(at.sum())
                if at.any():
                    st["node_instr"] += COST["visit"]
                    lane_pos[at] += 1
            budget -= NODE_UNROLL
            left = int((state() == NODE).sum())
            if not (budget > 0 and left >= keep):
                return left

    def swap():
        nonlocal nxt
        new = 0
        for i in range(64):
            s = lane_seq[i]
            if s is None or lane_pos[i] >= len(s):
                if nxt < len(seqs):
                    lane_seq[i], lane_pos[i] = seqs[nxt], 0
                    nxt += 1
                    new += 1
                else:
                    lane_seq[i] = None
        st["swap_runs"] += 1
        st["swap_lanes"] += new
        st["swap_instr"] += COST["swap"] + (COST["head"] if head and new else 0)

    tick, first = 0, False
    while True:
        known = -1
        while True:
            cur = state()
            n_n = known if known >= 0 else int((cur == NODE).sum())
            n_p = int((cur > NODE).sum())
            free = 64 - n_n - n_p
            if n_n + n_p == 0:
                break
            if not first:  # (the kernel's test short-circuits: the trip counter moves only where neither of the others decided)
                if free >= swap_min:
                    break
                tick += 1
                if (tick & 3) == 0:
                    break
            first = False
            if n_p >= prim_min or n_n == 0:
                left = prim_step()
                known = node_burst(left) if left >= FUSE_MIN else left
            else:
                known = node_burst(n_n)
        # what a swap would move, as the kernel counts it: finished walks out, and READY contexts into every lane without a walk
        n_f = sum(1 for i in range(64) if lane_seq[i] is not None and lane_pos[i] >= len(lane_seq[i]))
        if nxt + free > len(seqs):
            break  # the stream cannot fill this swap: the steady state ends here, the wave's drain is not part of it
        gain = n_f + free
        if gain >= swap_min:
            swap()
        elif n_p >= prim_min or (n_n == 0 and n_p > 0) or n_n > 0:
            first = True
        else:
            swap()
    # rays served, in-flight walks counted by the share of their steps that ran
    st["rays"] = (st["node_lanes"] + st["prim_lanes"]) / np.mean([len(s) for s in seqs])
    return st


def report(st, label):
    rays = max(1, st["rays"])
    total = st["node_instr"] + st["prim_instr"] + st["swap_instr"]
    print("%-10s %6.2f traversal instructions per ray: node %5.2f, primitive %5.2f, swap %5.2f; fill: node %4.1f lanes, primitive %4.1f, swap %4.1f new rays" % (
        label, total / rays, st["node_instr"] / rays, st["prim_instr"] / rays, st["swap_instr"] / rays,
        st["node_lanes"] / max(1, st["node_runs"]), st["prim_lanes"] / max(1, st["prim_runs"]), st["swap_lanes"] / max(1, st["swap_runs"])))
    return total / rays


def masterchief_sequences(count, seed=5, closest_inf=False):
    """(step sequences of `count` recorded rays of the headline frame at the oracle's final t -- closest_inf: at closest =
    +inf throughout, the other bracket of a real walk --, primitive tests of the head or None)"""
    import importlib
    import oracle.oracle_py as O
    import regroup_elide as E
    from test_regroup_host import _flat, _intervals, _recorded_rays, _regroup
    O.lib()
    srt = importlib.import_module("sexy-raytracer_amd")
    abi, dev = srt.abi, srt.device()
    sb = srt.scenes.scene_masterchief()
    sc = O.OracleScene(sb)
    rays = _recorded_rays(O, abi, sc, count, seed)[:count]
    hits = sc.trace(rays)
    t_final = np.where((hits["prim"] >= 0) & (not closest_inf), hits["t"], F(np.inf)).astype(F)
    rc, rg = _regroup(dev, _flat(sc.bvh(0)[0]), [0])
    assert rc == 1
    rc, _, src, links, entry = E.walk_host(dev, rg, [0])
    assert rc == 1
    sphere = np.concatenate(sb._prim_chunks)[:, 0] == abi.SRT_PRIM_SPHERE
    sphere_of = lambda ref: bool(sphere[~ref])  # noqa: E731  (the oracle's references: ~primitive)
    seqs = []
    for s in range(0, len(rays), 500):
        a, b, inside = _intervals(rg, rays[s:s + 500], gates=True)
        passes = inside & ~(np.fmin(b, t_final[s:s + 500, None]) <= a)
        seqs += step_sequences(rg, src, links, int(entry[0]), passes, sphere_of)
    return seqs, head_length(rg, src, sphere_of)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rays", type=int, default=3000)
    ap.add_argument("--head", action="store_true", help="model the head of the walks (tunable wf_head)")
    ap.add_argument("--prim-min", type=int, default=12)
    ap.add_argument("--swap-min", type=int, default=32)
    ap.add_argument("--keep-eighths", type=int, default=4)
    ap.add_argument("--prim-again-min", type=int, default=4)
    ap.add_argument("--closest-inf", action="store_true", help="walks at closest = +inf instead of the oracle's final t")
    args = ap.parse_args()
    seqs, head = masterchief_sequences(args.rays, closest_inf=args.closest_inf)
    n = np.array([[(s == k).sum() for k in (NODE, SPHERE, TRI)] for s in seqs]).mean(axis=0)
    print("%d rays: %.1f node visits, %.2f sphere tests, %.2f triangle tests per ray" % (len(seqs), n[0], n[1], n[2]))
    knobs = dict(prim_min=args.prim_min, swap_min=args.swap_min, keep_eighths=args.keep_eighths, prim_again_min=args.prim_again_min)
    base = report(simulate(seqs, **knobs), "baseline")
    if args.head:
        if head is None:
            print("the walks of this scene have no head")
            return
        with_head = report(simulate(take_head(seqs, head), head=True, **knobs), "head")
        print("head: %+.2f instructions per ray (%+.1f%%)" % (with_head - base, 100.0 * (with_head - base) / base))


if __name__ == "__main__":
    main()
