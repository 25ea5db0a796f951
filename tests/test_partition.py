"""csrc/pfc_partition.h, the rule by which a multi-device handle cuts its items into one contiguous range per shard:
tests/partition_check.cpp (its own main, includes only that header) is built by the host compiler with AddressSanitizer and
UBSan, every array allocated to the element, and run ONCE over all cases; nothing is loaded into Python.  Its output is compared
for equality with the statement in tests/partition_reference.py and held to properties that follow from the rule itself.

Cases: K in 1..8, n in 1..299, multi_min in {-1, 0, 1, 2, 8}, fixed seeds, the cost families: equal; uniform; heavy-tailed
(log-normal, sigma 2: single items dominate and both clamps bind); one item of 1e6 among items of 64; and costs shaped like
the two scaling configurations' counters.  (profiles/ records totals per run, no per-item counter array, so these are
synthetic: "c4" = scenes of one kind, 64 + t + 4 c with t in 30..60 node tests and c in 6..16 candidates; "c5" = pile pairs,
nine in ten apart (1 node test, no candidate: cost 65), the rest touching with 100..900 node tests and 10..120 candidates.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import partition_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")
FAMILIES = ("equal", "uniform", "heavy", "spike", "c4", "c5")
MIN_ITEMS = (-1, 0, 1, 2, 8)


def _costs(family, n, rng):
    if family == "equal":
        return [float(rng.choice([64.0, 64.0 + 0.02 * 12 * 200, 1.0, 1e-3]))] * n
    if family == "uniform":
        return list(64.0 + 1000.0 * rng.random(n))
    if family == "heavy":
        return list(64.0 + np.exp(2.0 * rng.standard_normal(n) + 4.0))
    if family == "spike":
        c = [64.0] * n
        c[int(rng.integers(n))] = 1e6
        return c
    if family == "c4":
        return [P.cost_counters(int(t), int(c)) for t, c in zip(rng.integers(30, 61, n), rng.integers(6, 17, n))]
    if family == "c5":
        touch = rng.random(n) < 0.1
        return [P.cost_counters(int(t), int(c)) if hit else P.cost_counters(1, 0)
                for hit, t, c in zip(touch, rng.integers(100, 901, n), rng.integers(10, 121, n))]
    raise KeyError(family)


def _cases():
    """(family, K, n, min_items, prev or None, cost): prev = (k_use, bound[0..K]) of an earlier evaluation of the same items."""
    out = []
    for K in range(1, 9):                      # the edges of n against K, every multi_min
        for mi in MIN_ITEMS:
            for n in sorted({1, 2, max(K - 1, 1), K, K + 1, 8 * K - 1, 8 * K, 8 * K + 1, 299}):
                out.append(("equal", K, n, mi, None, [64.0] * n))
    out.append(("equal", 8, 256, 8, None, [P.cost_leaves(12, 2)] * 256))       # 256 scenes over 8 shards
    out.append(("equal", 8, 2016, 8, None, [P.cost_leaves(12, 12)] * 2016))    # 2 016 pile pairs (the one case beyond n = 299)
    for f, family in enumerate(FAMILIES):
        rng = np.random.default_rng(1000 + f)
        for _ in range(650):
            K, n, mi = int(rng.integers(1, 9)), int(rng.integers(1, 300)), int(rng.choice(MIN_ITEMS))
            if rng.random() < 0.15:
                n = int(rng.integers(1, 2 * K + 2))        # few items per shard: n == k_use, idle shards
            cost = _costs(family, n, rng)
            prev = None
            if rng.random() < 0.5:                         # the ranges cut for slightly (or, one time in four, wholly) other costs
                other = _costs(family, n, rng) if rng.random() < 0.25 else [c * float(np.exp(0.1 * rng.standard_normal())) for c in cost]
                ku = P.k_use(n, K, mi if rng.random() < 0.9 else 1)
                prev = (ku, P.cut(other, ku, K))
            out.append((family, K, n, mi, prev, cost))
    return out


def _build(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build tests/partition_check.cpp")
    exe = str(tmp_path / "partition_check")
    # (g++: the sanitizer runtimes linked into the program, so that their place in the library order does not depend on the environment)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", *static, "-I", CSRC, os.path.join(ROOT, "tests", "partition_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def test_partition_rule_under_sanitizers(tmp_path):
    exe = _build(tmp_path)
    cases = _cases()
    assert 3000 < len(cases) < 6000
    lines = []
    for family, K, n, mi, prev, cost in cases:
        head = [K, n, mi, 0] if prev is None else [K, n, mi, 1, prev[0], *prev[1]]
        lines.append(" ".join([*map(str, head), *(float(c).hex() for c in cost)]))
    formulas = [(1, 1, 0, 0), (12, 200, 37, 9), (4096, 4096, 2 ** 31 - 1, 2 ** 31 - 1), (731, 1999, 123456, 7)]
    lines += ["c %d %d %d %d" % f for f in formulas]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == "", run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert got[-1] == "partition ok %d" % len(cases), got[-1]
    assert len(got) == len(cases) + len(formulas) + 1

    for f, line in zip(formulas, got[len(cases):]):
        c, leaves, counters = line.split()
        assert c == "c" and float.fromhex(leaves) == P.cost_leaves(f[0], f[1]) and float.fromhex(counters) == P.cost_counters(f[2], f[3]), (f, line)

    worst_ratio = dict.fromkeys(FAMILIES, 0.0)
    for (family, K, n, mi, prev, cost), line in zip(cases, got):
        head, b1, b2 = (list(map(int, part.split())) for part in line.split("|"))
        ku, keep_prev, keep_fresh = head
        tag = (family, K, n, mi, line)
        # --- the statement
        assert ku == P.k_use(n, K, mi) == max(1, min(K, n // max(mi, 1))), tag
        assert b1 == P.cut(cost, ku, K), tag
        assert keep_fresh == int(P.keeps(cost, b1, ku)), tag
        want_prev = -1 if prev is None or prev[0] != ku else int(P.keeps(cost, prev[1], ku))
        assert keep_prev == want_prev, tag
        # --- properties of the rule
        assert len(b1) == K + 1 and b1[0] == 0, tag
        assert all(b1[k] < b1[k + 1] for k in range(ku)), tag                      # every used shard has an item
        assert all(b1[k] == n for k in range(ku, K + 1)), tag                      # idle shards: empty ranges at the end
        if n == ku:
            assert b1[:ku + 1] == list(range(n + 1)), tag                          # one item per shard
        assert b2 == b1, tag                                                       # cutting twice gives the same bounds
        per = P.shard_costs(cost, b1, ku)
        total, top = sum(per), max(cost)
        # each boundary lies within half an item of its target (the half-item rule), so no range exceeds total / k_use by more than an item
        assert max(per) <= total / ku + top, (tag, max(per), total / ku, top)
        if top * ku <= 0.15 * total:                                               # ... and then the fresh cut passes its own 15 % rule
            assert keep_fresh == 1, tag
        worst_ratio[family] = max(worst_ratio[family], max(per) * ku / total)

    i256, i2016 = (next(i for i, c in enumerate(cases) if c[2] == n and c[1] == 8 and c[3] == 8 and c[0] == "equal") for n in (256, 2016))
    assert got[i256].split("|")[1].split() == [str(32 * k) for k in range(9)]
    assert got[i2016].split("|")[1].split() == [str(252 * k) for k in range(9)]
    # information for the reader, not an assertion: the worst shard's load over the mean after a fresh cut, per cost family
    print("worst (worst shard * k_use / total) of a fresh cut:", {f: round(float(r), 3) for f, r in worst_ratio.items()})
