"""The accept rule kept honest, every round, on a FIXED list: 2 001 pre-drawn cases of tools/fuzz_parity.py's
generator — seed 101, cases 1 .. 1 000 and 19 400 .. 20 400; the soak of round 5 found its one artefact pixel at case 19 899 —
stored as numbers in tests/golden/fuzz_cases_seed101.json by tools/draw_fuzz_cases.py.

Per case (scene kind and size, frame size, camera): the reference's frame (oracle, Raytracing.compute:89-103: min over every
computed t) against the frame under the fast modes' accept rule (`fast_rule`: a t in front of its own triangle's box does not
count).  They may differ ONLY at pixels where the reference's winner is such a t — checked pixel by pixel on the CPU
(oracle.unexplained_mismatches / winner_before_its_box) — and those pixels are COUNTED: the count is part of the test's output and
asserted (one pixel in these 2 001 cases: case 19 899's).  On the GPU the three modes are then compared with their frames:
LBVH_TRACE_REFERENCE == the reference frame word for word, LBVH_TRACE_FAST == the rule frame in t, LBVH_TRACE_FAST_EXACT == the
rule frame word for word."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as O                                                   # noqa: E402
from query_support import words                                      # noqa: E402
from unitysimpleraytracing_amd import layouts as L, scenes           # noqa: E402

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz_cases_seed101.json")))
CASES = FIXTURE["cases"]


def make_scene(kind, n, p):
    """tools/fuzz_parity.py make_scene (the fixture holds the draws, this turns them into triangles)"""
    if kind == "soup":
        return scenes.random_triangles(n, seed=p["seed"])
    if kind == "torus":
        return scenes.tiled_torus(nu=p["nu"], nv=p["nv"], grid=p["grid"], seed=p["seed"])
    t = scenes.random_triangles(n, seed=p["seed"])
    if kind == "dups":
        k = max(n // 4, 1)
        t[k:2 * k] = t[:k][: len(t[k:2 * k])]
        t[2 * k:3 * k] = t[:k][: len(t[2 * k:3 * k])]
        for f in ("a", "b", "c"):
            t[f][3 * k:] = t[f][3 * k:] * np.float32(1e-3)
    elif kind == "one_cell":
        for f in ("a", "b", "c"):
            t[f] = t[f] * np.float32(1e-4) + np.float32(17.0)
    elif kind == "slivers":
        t["b"] = t["a"] + (t["b"] - t["a"]) * np.float32(1e-6)
    elif kind == "outside":
        for f in ("a", "b", "c"):
            t[f] = t[f] * np.float32(3.0)
    return t


def camera_of(q):
    cam = dict(q["cam"])
    cam["camera_to_world"] = np.array(cam["camera_to_world"], dtype=np.float32)
    return cam


def oracle_pair(q, threads):
    """(triangles, camera, built, reference frame, rule frame, artefact pixels) of one case; raises on an unexplained difference"""
    tris = make_scene(q["kind"], q["n"], q["scene"])
    cam = camera_of(q)
    b = O.Built(tris, threads=threads)
    oh, _ = O.trace_primary(b, cam, threads=threads)
    of, _ = O.trace_primary(b, cam, threads=threads, fast_rule=True)
    explained = []
    if not (words(oh) == words(of)).all():
        unexplained, explained = O.unexplained_mismatches(b, cam, oh, of, words=True)
        assert not unexplained, (q["case"], "reference frame vs rule frame differ where the winner is NOT in front of its box", unexplained[:4])
    return tris, cam, b, oh, of, explained


def test_the_fixture_is_the_generators_case_list():
    assert FIXTURE["seed"] == 101 and len(CASES) == 2001
    numbers = [q["case"] for q in CASES]
    assert numbers == list(range(1, 1001)) + list(range(19400, 20401))
    q = [q for q in CASES if q["case"] == 19899][0]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "grazing_ray_case.json")))
    assert q["kind"] == "torus" and q["scene"] == {k: pinned["scene"][k] for k in ("nu", "nv", "grid", "seed")}
    assert (q["w"], q["h"]) == (pinned["w"], pinned["h"])
    assert np.allclose(q["cam"]["camera_to_world"], pinned["camera"]["camera_to_world"])
    assert len({q["kind"] for q in CASES}) == 6


def test_oracle_frames_differ_only_where_the_winner_lies_before_its_box_cpu_subset():
    """CPU suite: every 16th case and the pinned one (the whole list runs with the GPU suite)"""
    subset = [q for q in CASES if q["case"] % 16 == 0 or q["case"] == 19899]
    artefacts = {}
    for q in subset:
        _, _, _, _, _, explained = oracle_pair(q, O.num_threads())
        if explained:
            artefacts[q["case"]] = explained
    assert artefacts == {19899: [(12, 210)]}, artefacts


def _oracle_job(q):
    """one case's oracle side in a worker process (no HIP in there): frames and artefact pixels"""
    _, _, _, oh, of, explained = oracle_pair(q, 4)
    return q["case"], oh, of, explained


@pytest.mark.gpu
def test_fixed_fuzz_cases_reference_frame_vs_rule_frame_and_the_three_modes(ctx):
    """all 2 001 cases.  The oracle's two frames per case come from a pool of worker processes (spawned: they never touch HIP;
    serial with 8 threads the CPU side alone took 20 minutes on the GPU box), the GPU's three modes are compared as they arrive."""
    import concurrent.futures as cf
    import multiprocessing as mp
    from unitysimpleraytracing_amd.host import RaytracingMeshDrawer
    artefacts = {}
    pixels = 0
    workers = max(2, min(24, (os.cpu_count() or 8) // 4))
    with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as pool:
        for q, (case, oh, of, explained) in zip(CASES, pool.map(_oracle_job, CASES, chunksize=8)):
            assert case == q["case"]
            if explained:
                artefacts[case] = explained
            pixels += oh.size
            tris, cam = make_scene(q["kind"], q["n"], q["scene"]), camera_of(q)
            d = RaytracingMeshDrawer(ctx, tris).awake(fast=True)
            what = (q["case"], q["kind"], len(tris), q["w"], q["h"])
            d.update(cam, mode=L.TRACE_REFERENCE)
            assert (words(d.hits()) == words(oh)).all(), what + ("reference mode",)
            for frame in range(2):                     # the second frame runs the dispatch history of the first
                d.update(cam, mode=L.TRACE_FAST)
                assert (d.hits()["t"] == of["t"]).all(), what + ("fast mode", frame)
            d.update(cam, mode=L.TRACE_FAST_EXACT)
            assert (words(d.hits()) == words(of)).all(), what + ("exact mode",)
            d.on_destroy()
    print(f"\n{len(CASES)} fixed fuzz cases, {pixels} pixels: reference frame vs rule frame differ at {sum(map(len, artefacts.values()))} "
          f"pixel(s), every one a winner in front of its own triangle's box: {artefacts}")
    assert artefacts == {19899: [(12, 210)]}, artefacts
