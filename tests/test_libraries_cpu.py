"""The structure every native library shares, checked once for every row of sslam_amd.lib.LIBRARIES: the header, the dynamic symbols
of the built shared object and the export list hold the same entries; the library loads, and a missing one is an error; it is rebuilt
only when a prerequisite is newer; its directory holds what is pinned here; the prerequisites stated in its Makefile, in its row and
by the #include lines of its sources agree; and __graft_entry__.build() makes the table's directories in the table's order.
A new library adds a row to ENTRIES, VERSION and FILES below, and to nothing else in tests/.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from sslam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(lib.LIBRARIES.values())
MK = [os.path.join(lib.CSRC, "flags.mk"), os.path.join(lib.CSRC, "rules.mk")]
# the number of entries each header declares, and the lowest version each library reports
ENTRIES = dict(lib=81, ext=4, graph=6, loop=7, window=5, place=6, conf=9, weight=5, track=8)
VERSION = dict(lib=650, ext=100, graph=100, loop=100, window=100, place=100, conf=100, weight=100, track=100)
# exported without a declaration in the header: the test hooks of the first library's border plan (sslam_amd.lib.selector_border_*)
INTERNAL = dict(lib={"sslami_selector_border_plan", "sslami_selector_border_check", "sslami_selector_border_owners"})
# what each directory holds beside its Makefile, build products aside
FILES = dict(
    lib=["bn_tokens.hip", "common.h", "evaluate.hip", "flags.mk", "gather_taps.h", "lib.hip", "match.hip", "pose_common.h", "pose_estimate.hip",
         "pose_refine.hip", "pose_refine_common.h", "rank.hip", "refine.hip", "refine_bf16.hip", "resample.hip", "rules.mk", "select.hip",
         "selector.hip", "selector_bf16.hip", "validate.hip", "vit.hip", "vit_f32.hip"],
    ext=["subcell.hip"], graph=["edge_terms.h", "edge_walk.h", "gauss_newton.h", "pose_graph.hip"], loop=["loop.hip"], window=["window.hip"],
    place=["place.hip"], conf=["confidence.hip"], weight=["weighted_refine.hip"], track=["track.hip"])
# words of one feature that the entry names of other libraries do not carry: (the rows looked at, the words)
FOREIGN_WORDS = ((("lib",), ("subcell",)), (("lib", "ext"), ("graph",)), (("lib", "ext", "graph"), ("loop", "sparse")),
                 (("window",), ("graph", "loop", "sparse", "subcell")),
                 (("place",), ("graph", "sparse", "window", "subcell", "candidates", "signatures")))
by_name = pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])


def declared(row):
    """The entries the row's header declares, its comments dropped."""
    text = re.sub(r"/\*.*?\*/", " ", open(row.header_path).read(), flags=re.S)
    return re.findall(r"^(?:int|long long|size_t|const char \*)\s*(" + row.prefix + r"_\w+)\s*\(", text, flags=re.M)


def sources(row):
    return [os.path.join(row.csrc, f) for f in sorted(os.listdir(row.csrc)) if f.endswith((".hip", ".h"))]


# ------------------------------------------------------------------------------------------------- header, symbols and exports
@by_name
def test_header_symbols_and_exports_agree(row):
    names = declared(row)
    assert len(set(names)) == len(names) == ENTRIES[row.name]
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm to list the library's dynamic symbols with"
    dyn = subprocess.run([nm, "-D", "--defined-only", row.so_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT\s+(\w+)$", dyn, flags=re.M))
    # nothing but the declared entries leaves the library, the pinned hooks aside
    assert exported == set(names) | INTERNAL.get(row.name, set()), sorted(exported ^ set(names))
    assert set(row.exports) == set(names) and len(set(row.exports)) == len(row.exports)
    assert all(n.startswith(row.prefix + "_") for n in row.exports)


def test_no_library_carries_anothers_entries():
    assert list(lib.LIBRARIES) == list(ENTRIES) == list(FILES) == list(VERSION)
    assert len({r.prefix for r in ROWS}) == len({r.so_path for r in ROWS}) == len({r.csrc for r in ROWS}) == len({r.header for r in ROWS}) == len(ROWS)
    for i, a in enumerate(ROWS):
        for b in ROWS[i + 1:]:
            assert not set(a.exports) & set(b.exports), (a.name, b.name)
            # a header may speak of the libraries its own builds on, never of a later one
            assert b.prefix + "_" not in open(a.header_path).read(), (a.header, b.prefix)
    for names, words in FOREIGN_WORDS:
        carried = [n for name in names for n in lib.LIBRARIES[name].exports if any(w in n for w in words)]
        assert not carried, (names, carried)
    assert "subcell" not in open(lib.LIBRARIES["lib"].header_path).read()
    # the names the rest of the tree uses are the table's
    assert lib.SO_PATH == lib.LIBRARIES["lib"].so_path and lib.CSRC == lib.LIBRARIES["lib"].csrc and lib.EXPORTS is lib.LIBRARIES["lib"].exports
    for r in ROWS[1:]:
        assert getattr(lib, r.name.upper() + "_EXPORTS") is r.exports, r.name


# --------------------------------------------------------------------------------------------------------------------- loading
@by_name
def test_the_library_loads_and_reports_its_target(row):
    L = row.load()
    assert L is row.load() is getattr(lib, row.name)(), "loaded once, and the module's loader is the row's"
    assert all(hasattr(L, name) for name in row.exports)
    assert getattr(L, row.prefix + "_arch")() == b"gfx950" and getattr(L, row.prefix + "_version")() >= VERSION[row.name]
    assert row.launch_count() >= 0
    count = getattr(lib, "launch_count" if row.name == "lib" else row.name + "_launch_count")
    assert count() == row.launch_count()


@by_name
def test_a_missing_library_is_an_error(row, monkeypatch, tmp_path):
    monkeypatch.setattr(row, "handle", None)
    monkeypatch.setattr(row, "so_path", str(tmp_path / row.so))
    with pytest.raises(lib.SslamHipError, match="missing: run"):
        row.load()
    with pytest.raises(lib.SslamHipError, match="missing: run"):
        getattr(lib, row.name)()


# ------------------------------------------------------------------------------------------------------------------- staleness
@by_name
def test_build_rebuilds_only_a_stale_library(row, monkeypatch):
    calls = []
    monkeypatch.setattr(lib.subprocess, "check_call", lambda cmd, **kw: calls.append(cmd))
    build = getattr(lib, "build" if row.name == "lib" else row.name + "_build")
    assert row.build() == build() == row.so_path and calls == [], "an up-to-date library is left alone"
    build(force=True)
    assert calls == [["make", "-C", row.csrc, "-s", "-j4"]]
    real = os.path.getmtime
    prerequisites = sources(row) + row.prerequisites + MK
    assert len(set(prerequisites)) == len(prerequisites)
    for n, newer in enumerate(prerequisites):
        monkeypatch.setattr(lib.os.path, "getmtime", lambda p, newer=newer: real(p) + (1e6 if p == newer else 0))
        build()
        assert calls == [["make", "-C", row.csrc, "-s", "-j4"]] * (2 + n), newer


# ---------------------------------------------------------------------------------------------------------- directory contents
@by_name
def test_the_directory_holds_what_is_pinned(row):
    held = sorted(f for f in os.listdir(row.csrc) if not f.startswith("_") and not f.endswith(".so"))
    assert held == sorted(FILES[row.name] + ["Makefile"])


def test_the_source_directories_are_the_tables():
    package = os.path.dirname(lib.CSRC)
    assert sorted(d for d in os.listdir(package) if d.startswith("csrc")) == sorted(r.directory for r in ROWS)
    assert all(r.csrc == os.path.join(package, r.directory) and os.path.dirname(r.so_path) == r.csrc for r in ROWS)
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(r.header for r in ROWS)


# ---------------------------------------------------------------------------------------------------------- the prerequisites
def included(path, seen):
    """Every file reached from `path` through #include "..." lines, each resolved relative to the file that includes it."""
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        target = os.path.normpath(os.path.join(os.path.dirname(path), name))
        if target not in seen:
            seen.add(target)
            included(target, seen)
    return seen


@by_name
def test_makefile_row_and_includes_name_the_same_prerequisites(row):
    lines = open(os.path.join(row.csrc, "Makefile")).read().splitlines()
    assert len(lines) == 3 and lines[0].split() == ["OUT", ":=", row.so] and lines[2] == "include ../csrc/rules.mk"
    assert lines[1].split()[:2] == ["DEPS", ":="]
    deps = [os.path.normpath(os.path.join(row.csrc, d)) for d in lines[1].split()[2:]]
    assert deps == row.prerequisites and len(set(deps)) == len(deps)
    assert row.header_path in deps and all(os.path.dirname(d) != row.csrc for d in deps)
    reached = set()
    for src in sources(row):
        if src.endswith(".hip"):
            included(src, reached)
    outside = {f for f in reached if os.path.dirname(f) != row.csrc}
    assert outside == set(deps), (sorted(outside - set(deps)), sorted(set(deps) - outside))     # none missing, none stale
    inside = reached - outside
    assert inside <= set(sources(row)) and {s for s in sources(row) if s.endswith(".h")} <= inside, "every header of the directory is used"


# ------------------------------------------------------------------------------------------------------------ the build driver
def test_graft_entry_makes_the_tables_directories_in_order(monkeypatch):
    import __graft_entry__ as entry
    calls = []
    monkeypatch.setattr(entry.subprocess, "check_call", lambda cmd, **kw: calls.append(cmd))
    entry.build()
    n = len(ROWS)
    assert calls[:n] == [["make", "-C", r.csrc, "-s", "-j4"] for r in ROWS]
    assert calls[n] == ["make", "-C", os.path.join(ROOT, "oracle"), "-s"]
    assert not [c for c in calls[n:] if c[0] == "make" and "csrc" in c[2]]
    assert [r.directory for r in ROWS] == ["csrc", "csrc_ext", "csrc_graph", "csrc_loop", "csrc_window", "csrc_place", "csrc_conf", "csrc_weight",
                                           "csrc_track"]
