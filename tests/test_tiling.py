"""hp_tiling.hpp: how every flux launch is cut into row bands and tiles (choose_tiling, make_tile_map), pinned without a GPU.

tests/tiling_probe.cpp is compiled with plain g++ and run over the cases of tests/tiling_table.json; what it prints must be
the table.  The table was NOT made with this header: it was generated once from the policy as it stood inside
hp_domain_create, and from make_tile_map as it stood in hp_engine.hip, before both moved here -- the two blocks pasted
verbatim into a throw-away harness that ran one process per case with the knobs in its environment.  It therefore holds
every decision of the engine at that commit; a change of any tiling number shows up here as a changed row, which is then
either a bug or a deliberate change that regenerates the row from the new header and says so."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = json.load(open(os.path.join(HERE, "tiling_table.json")))

# the shapes (cols, rows) that the comments of the policy cite
SHAPES = [(3, 3), (64, 64), (342, 195), (512, 512), (1024, 1024), (1448, 1448), (2048, 2048), (4096, 4096), (8192, 8192),
          (4096, 514), (4096, 516), (3072, 514), (4096, 1026), (8192, 514), (8192, 1026), (8192, 2050), (16384, 1026), (16384, 8192)]
KNOB_ROWS = [{"HP_TILING_SEARCH": "0"}, {"HP_RSEG_REFINE": "0"}, {"HP_MARCH_RSEG": "16"}, {"HP_MARCH2_RSEG": "20"}, {"HP_NBANDS": "12"}]


def case_id(e):
    knobs = ",".join(f"{k}={v}" for k, v in e["knobs"].items())
    return f"{e['cols']}x{e['rows']}-fp{8 * e['precision']}-{e['cus']}cu" + (f"-{knobs}" if knobs else "")


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tiling") / "tiling_probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "tiling_probe.cpp")])
    lines = "".join("%d %d %d %d %d %s\n" % (e["cols"], e["rows"], e["precision"], e["cus"], e["strip"],
                                             " ".join(f"{k}={v}" for k, v in e["knobs"].items())) for e in TABLE)
    out = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    return [json.loads(l) for l in out]


def test_the_header_needs_no_hip_and_reads_no_environment():
    text = open(os.path.join(CSRC, "hp_tiling.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "getenv" not in code and "#include <hip" not in code and "hip/" not in code


def test_table_covers_the_cited_shapes_and_the_knobs():
    rows = {(e["cols"], e["rows"], e["precision"], e["cus"], json.dumps(e["knobs"], sort_keys=True)) for e in TABLE}
    for i, (c, r) in enumerate(SHAPES):
        for p in (8, 4):
            assert (c, r, p, 256, "{}") in rows
            assert i % 3 or (c, r, p, 64, "{}") in rows                   # a third of the shapes on a 64-CU device
        for k in KNOB_ROWS:
            assert (c, r, 8, 256, json.dumps(k, sort_keys=True)) in rows
    for e in TABLE:
        kinds = {(m["kernel"], m["part"]) for m in e["maps"]}
        assert {("K1", "all"), ("pair", "all")} <= kinds and (e["rows"] <= 4 or ("K2", "all") in kinds)
        if e["rows"] in (514, 516, 1026, 2050):                             # the strips of a decomposed run
            assert e["strip"] and {("K1", "interior"), ("K1", "halo"), ("K2", "interior"), ("K2", "halo")} <= kinds
    searched = [e for e in TABLE if e["tiling"]["march_nbands"] != 8 or e["tiling"]["march2_nbands"] != 8]
    assert len(searched) >= 20                                              # the one-round search decides a good part of it


@pytest.mark.parametrize("index", range(len(TABLE)), ids=[case_id(e) for e in TABLE])
def test_tiling_is_the_table(probed, index):
    want, got = TABLE[index], probed[index]
    assert got["tiling"] == want["tiling"]
    assert got["maps"] == want["maps"]


@pytest.mark.parametrize("index", range(len(TABLE)), ids=[case_id(e) for e in TABLE])
def test_tile_maps_cover_their_rows(index):
    """Every launch of the table has a tile for each of its rows and a block for each of its tiles (tile_rows of hp_kernels.hpp
    reads exactly these fields)."""
    for m in TABLE[index]["maps"]:
        if not m["made"]:
            continue
        rows = m["y_end"] - m["y_begin"]
        assert m["rseg"] <= m["band_rows"]
        assert m["nbig"] * m["rseg"] + m["ntail"] * m["rseg_tail"] >= m["band_rows"]
        if m["part"] == "halo" and m["nbands"] == 2:                        # a south and a north block of band_rows rows
            assert m["band_stride"] + m["band_rows"] == rows and 2 * m["band_rows"] < rows and m["ntail"] == 0
            assert m["blocks"] == 2 * m["groups"] * m["nbig"]
        else:
            assert m["band_stride"] == m["band_rows"] and m["nbands"] * m["band_rows"] >= rows
            assert m["blocks"] == m["nbands"] * m["groups"] * (m["nbig"] + m["ntail"])
        assert m["groups"] * 4 >= m["nstrips"]
