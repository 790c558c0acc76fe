"""hp_order.hpp: in which order a band's blocks of a pair launch take its tiles, pinned without a GPU.

tests/order_probe.cpp is compiled with plain g++.  Its sweep holds every table -- groups 1..20, row segments 1..23, every flag mask up
to 10 groups and 200 seeded ones above, one 64-group case -- against the order's definition built the long way round: a bijection onto
groups x segments, every flagged group's tile in front of every other tile, tile-row by tile-row within each class with the groups
ascending, and exactly `i % groups, i / groups` where no group or every group is flagged.  The small tables are checked once more here,
from the probe's printed words, by code that shares nothing with the header."""
import itertools
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("order") / "order_probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "order_probe.cpp")])
    return str(exe)


def tables(probe, cases):
    lines = "".join("%d %d %d\n" % c for c in cases)
    out = subprocess.run([probe, "tables"], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [[tuple(int(v) for v in w.split(":")) for w in l.split()] for l in out]


def by_definition(groups, nseg, mask):
    flagged = [g for g in range(groups) if (mask >> g) & 1]
    others = [g for g in range(groups) if not (mask >> g) & 1]
    if not flagged or not others:
        return [(i % groups, i // groups) for i in range(groups * nseg)]
    return [(g, s) for s in range(nseg) for g in flagged] + [(g, s) for s in range(nseg) for g in others]


def test_the_header_needs_no_hip_and_keeps_no_state():
    text = open(os.path.join(CSRC, "hp_order.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "getenv" not in code and "#include" not in code and "static " not in code.replace("static inline", "")


def test_every_table_of_the_sweep_is_the_defined_permutation(probe):
    got = json.loads(subprocess.run([probe, "sweep"], capture_output=True, text=True, check=True).stdout)
    exhaustive = sum(23 * 2 ** g for g in range(1, 11))
    assert got["cases"] == exhaustive + 10 * 23 * 202 + 7
    assert got["bad"] == []


def test_small_tables_word_by_word(probe):
    cases = [(g, s, m) for g in range(1, 7) for s in (1, 2, 5) for m in range(2 ** g)]
    for (g, s, m), table in zip(cases, tables(probe, cases)):
        assert table == by_definition(g, s, m), (g, s, m)
        assert sorted(table) == sorted(itertools.product(range(g), range(s)))
        n_flagged = bin(m).count("1") * s
        if 0 < n_flagged < g * s:
            assert all((m >> gg) & 1 for gg, _ in table[:n_flagged]) and not any((m >> gg) & 1 for gg, _ in table[n_flagged:])


def test_no_hint_and_a_full_one_are_tile_row_by_tile_row(probe):
    cases = [(g, s, m) for g, s in ((1, 1), (3, 6), (18, 22), (20, 23), (64, 7)) for m in (0, 2 ** g - 1)]
    cases.append((18, 22, (2 ** 18 - 1) << 18))                      # bits beyond the groups: no group of this band is flagged
    for (g, s, m), table in zip(cases, tables(probe, cases)):
        assert table == [(i % g, i // g) for i in range(g * s)], (g, s, m)


def test_sixty_four_groups(probe):
    masks = [1 << 63, (1 << 63) | 1, 0xFFFF0000, (2 ** 64 - 1) ^ (1 << 31)]
    cases = [(64, 7, m) for m in masks]
    for (g, s, m), table in zip(cases, tables(probe, cases)):
        assert table == by_definition(g, s, m), hex(m)
        assert len(set(table)) == g * s


def test_the_headline_shape_puts_the_dam_groups_first(probe):
    # 4096^2: 18 groups x 22 tile rows per band; the groups around the dam flagged
    (table,) = tables(probe, [(18, 22, 0b111 << 8)])
    assert table[:6] == [(8, 0), (9, 0), (10, 0), (8, 1), (9, 1), (10, 1)]
    assert table[66:69] == [(0, 0), (1, 0), (2, 0)] and table[-1] == (17, 21)
