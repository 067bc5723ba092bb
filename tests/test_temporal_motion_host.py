"""The motion table of the temporal pass (ray_tracer_amd/csrc/temporal_motion.h) on the CPU: tests/temporal_motion_check.cpp,
built from temporal_motion.cpp with plain g++ (no hipcc, no HIP runtime, no device), runs its worked cases (flags for unmoved,
translated, rescaled and re-pointed objects, growing and shrinking counts, spheres moved and resized) and then turns the random
snapshot pairs this file writes into tables, whose flags, counts and matrices are checked here: D = Fwd' Inv and
G = Inv'^T Fwd^T against a numpy float64 product of the same fp32 rows, each entry within 2^-23 x the sum of the magnitudes of
its terms (one rounding to fp32 of a sum accumulated exactly, with room for the double accumulation's own last bits)."""
import numpy as np
import pytest

import hostcheck

UNMOVED, MOVED, REPLACED = 0, 1, 2


@pytest.fixture(scope="module")
def checker(tmp_path_factory, built):
    return hostcheck.build(tmp_path_factory.mktemp("temporal_motion"), "temporal_motion_check", ["temporal_motion.cpp"], "temporal_motion_check.cpp")


def test_worked_cases(checker):
    hostcheck.run(checker, ok="temporal motion ok")


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def random_object(rng, kind):
    """(fwd rows, inv rows) as fp32 (3, 4) arrays: the inverse is numpy's, rounded; the unit takes both as given."""
    m = np.eye(4)
    if kind == "translated":
        m[:3, 3] = rng.uniform(-3, 3, 3)
    elif kind == "rotated":
        m[:3, :3], m[:3, 3] = rotation(rng), rng.uniform(-3, 3, 3)
    elif kind == "rescaled":
        m[:3, :3], m[:3, 3] = rotation(rng) @ np.diag(rng.uniform(0.2, 4.0, 3)), rng.uniform(-3, 3, 3)
    f = m.astype(np.float32)
    return f[:3], np.linalg.inv(f.astype(np.float64)).astype(np.float32)[:3]


def words(a):
    return " ".join(f"{int(w):08x}" for w in np.ascontiguousarray(a).view(np.uint32).ravel())


def write_case(fh, prev, now, sprev, snow):
    fh.write(f"{len(prev)} {len(now)} {len(sprev)} {len(snow)}\n")
    for objs in (prev, now):
        for f, i, bvh in objs:
            fh.write(words(f) + " " + words(i) + f" {bvh:08x}\n")
    for sph in (sprev, snow):
        for s in sph:
            fh.write(words(np.asarray(s, np.float32)) + "\n")


def read_table(lines):
    head = [int(x) for x in next(lines).split()]
    objects = [np.array([int(w, 16) for w in next(lines).split()], np.uint32).reshape(7, 4) for _ in range(head[0])]
    spheres = [np.array([int(w, 16) for w in next(lines).split()], np.uint32).reshape(2, 4) for _ in range(head[1])]
    return head, objects, spheres


def expected_matrices(fp, ip, fn, inn):
    """D = Fwd' Inv (3 x 4) and G = Inv'^T Fwd^T (3 x 3) in float64 from the fp32 rows, each with the sum of its terms' magnitudes."""
    fp, ip, fn, inn = (np.asarray(x, np.float64) for x in (fp, ip, fn, inn))
    D = fp[:, :3] @ inn
    D[:, 3] += fp[:, 3]
    aD = np.abs(fp[:, :3]) @ np.abs(inn)
    aD[:, 3] += np.abs(fp[:, 3])
    G = ip[:, :3].T @ fn[:, :3].T
    aG = np.abs(ip[:, :3]).T @ np.abs(fn[:, :3]).T
    return D, aD, G, aG


def test_random_snapshots_against_float64(checker, tmp_path):
    rng = np.random.default_rng(20)
    kinds = ["unmoved", "translated", "rotated", "rescaled", "repointed"]
    cases = []
    for c in range(24):
        n_prev, n_now = (int(x) for x in rng.integers(0, 9, 2))
        s_prev, s_now = (int(x) for x in rng.integers(0, 6, 2))
        prev = [random_object(rng, kinds[int(rng.integers(1, 4))]) + (int(rng.integers(0, 50)),) for _ in range(n_prev)]
        now, what = [], []
        for o in range(n_now):
            k = kinds[(o + c) % len(kinds)] if o < n_prev else "new"
            what.append(k)
            if k == "unmoved":
                now.append(prev[o])
            elif k == "repointed":
                now.append(random_object(rng, "rotated") + (prev[o][2] + 1,))
            else:
                now.append(random_object(rng, k if k != "new" else "rescaled") + (prev[o][2] if o < n_prev else 3,))
        sprev = [np.append(rng.uniform(-2, 2, 3), rng.uniform(0.1, 2)).astype(np.float32) for _ in range(s_prev)]
        snow, swhat = [], []
        for s in range(s_now):
            k = ("unmoved", "moved", "resized")[(s + c) % 3] if s < s_prev else "new"
            swhat.append(k)
            v = sprev[s].copy() if s < s_prev else np.append(rng.uniform(-2, 2, 3), rng.uniform(0.1, 2)).astype(np.float32)
            if k == "moved":
                v[:3] += rng.uniform(0.01, 1, 3).astype(np.float32)
            if k == "resized":
                v[3] *= np.float32(rng.uniform(1.1, 3))
            snow.append(v)
        cases.append((prev, now, what, sprev, snow, swhat))
    src, out = tmp_path / "cases.txt", tmp_path / "tables.txt"
    with open(src, "w") as fh:
        for prev, now, what, sprev, snow, swhat in cases:
            write_case(fh, prev, now, sprev, snow)
    hostcheck.run(checker, [src, out], ok=f"{len(cases)} cases")
    lines = iter(open(out).read().splitlines())
    worst = 0.0
    seen = set()
    for c, (prev, now, what, sprev, snow, swhat) in enumerate(cases):
        head, objects, spheres = read_table(lines)
        grow, sgrow = abs(len(prev) - len(now)), abs(len(sprev) - len(snow))
        want = dict(moved=sum(k in ("translated", "rotated", "rescaled") for k in what), replaced=what.count("repointed") + grow,
                    smoved=sum(k in ("moved", "resized") for k in swhat), sreplaced=sgrow)
        assert head == [len(now), len(snow), want["moved"], want["replaced"], want["smoved"], want["sreplaced"]], (c, head, want)
        for o, (rec, k) in enumerate(zip(objects, what)):
            seen.add(k)
            flag = {"unmoved": UNMOVED, "repointed": REPLACED, "new": REPLACED}.get(k, MOVED)
            assert rec[0, 0] == flag and not rec[0, 1:].any(), (c, o, k, rec[0])
            if flag != MOVED:
                assert not rec[1:].any(), (c, o, k)
                continue
            D, aD, G, aG = expected_matrices(prev[o][0], prev[o][1], now[o][0], now[o][1])
            got = rec[1:].view(np.float32).astype(np.float64)
            assert (np.abs(got[:3] - D) <= 2.0 ** -23 * aD).all(), (c, o, k, got[:3], D)
            assert (np.abs(got[3:, :3] - G) <= 2.0 ** -23 * aG).all() and not rec[4:, 3].any(), (c, o, k, got[3:], G)
            worst = max(worst, float((np.abs(got[:3] - D) / np.maximum(aD, 1e-300)).max()), float((np.abs(got[3:, :3] - G) / np.maximum(aG, 1e-300)).max()))
            # what the pair is for: D takes a point placed now to where the previous placement had it, G is D's inverse transpose
            x = rng.uniform(-1, 1, 3)
            now_w = np.asarray(now[o][0], np.float64) @ np.append(x, 1.0)
            prev_w = np.asarray(prev[o][0], np.float64) @ np.append(x, 1.0)
            np.testing.assert_allclose(got[:3] @ np.append(now_w, 1.0), prev_w, atol=2e-4)
            np.testing.assert_allclose(got[3:, :3] @ got[:3, :3].T, np.eye(3), atol=2e-4)
        for s, (rec, k) in enumerate(zip(spheres, swhat)):
            seen.add("sphere " + k)
            flag = {"unmoved": UNMOVED, "new": REPLACED}.get(k, MOVED)
            assert rec[1, 3] == flag, (c, s, k, rec)
            if flag != MOVED:
                assert not rec[0].any() and not rec[1, :3].any(), (c, s, k)
                continue
            assert np.array_equal(rec[0, :3], snow[s][:3].view(np.uint32)) and np.array_equal(rec[1, :3], sprev[s][:3].view(np.uint32))
            assert rec[0, 3:].view(np.float32)[0] == np.float32(np.float64(sprev[s][3]) / np.float64(snow[s][3]))
    assert seen >= set(kinds) | {"new", "sphere unmoved", "sphere moved", "sphere resized", "sphere new"}, seen
    print(f"worst |entry - float64| / sum|terms|: {worst:.3g} (bound 2^-23 = {2.0 ** -23:.3g})")
