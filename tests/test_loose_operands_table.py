"""Nothing forgotten: every entry libsslam_hip.so exports (sslam_amd.lib.EXPORTS) is a row of tests/loose_table.py - and so run by
tests/test_gpu_loose_operands.py at its loosest alignment and stride - or one of the host-only entries, which take no device pointer.
A new entry fails here until it gets a row.  The table is also what include/sslam_hip.h states, argument for argument."""
import os
import re

import loose_table as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_hip.h")


def _exports():
    from sslam_amd import lib
    return list(lib.EXPORTS)


def test_every_export_is_a_row_or_host_only():
    exports = _exports()
    assert len(set(exports)) == len(exports)
    rows, host = set(lt.ALIGN), set(lt.HOST_ONLY)
    assert not rows & host, sorted(rows & host)
    missing = [name for name in exports if name not in rows and name not in host]
    assert not missing, f"entries without a row in tests/loose_table.py: {missing}"
    stale = sorted((rows | host) - set(exports))
    assert not stale, f"rows of entries that are not exported: {stale}"


def test_the_host_only_list_holds_host_only_entries():
    for name in lt.HOST_ONLY:
        assert lt.is_host_only_name(name), f"{name} is no packer, layout, size, version or knob entry: it needs a row"
    assert len(set(lt.HOST_ONLY)) == len(lt.HOST_ONLY)


def _prototypes():
    """entry -> [(type, name)] of its arguments, from the header."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|long long|const char \*)\s*(sslam_\w+)\s*\(([^;{]*?)\)\s*;", text):
        args = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            if a and a != "void":
                am = re.match(r"(.*?)(\w+)$", a)
                args.append((am.group(1).strip(), am.group(2)))
        out[m.group(1)] = args
    return out


def test_a_row_names_exactly_the_device_pointers_of_its_prototype():
    protos = _prototypes()
    elem = {"uint8_t": 1, "uint16_t": 2, "int32_t": 4, "float": 4, "int64_t": 8, "double": 8}
    for entry, row in lt.ALIGN.items():
        assert entry in protos, entry
        pointers = [(t, n) for t, n in protos[entry] if "*" in t and n != "stream" and not n.endswith("_host") and "weights" not in n]
        assert sorted(n for _, n in pointers) == sorted(row), (entry, sorted(set(n for _, n in pointers) ^ set(row)))
        for t, n in pointers:
            a = row[n]
            assert a in (1, 2, 4, 8, 16), (entry, n, a)
            base = t.replace("const", "").replace("*", "").strip()
            if base in elem:
                assert a >= elem[base], f"{entry}: {n} is a {base} array, its alignment cannot be below {elem[base]}"
        names = [n for _, n in protos[entry]]
        for s in lt.STRIDES.get(entry, ()):
            assert s in names, (entry, s)
        assert [n for t, n in protos[entry] if t == "long long" and "stride" in n] == list(lt.STRIDES.get(entry, ())), entry
    for entry in lt.HOST_ONLY:
        device = [n for t, n in protos.get(entry, []) if "*" in t and not n.endswith("_host") and n not in ("name", "w", "out", "w_up", "w_down",
                                                                                                          "row_scale", "L")]
        assert not device, (entry, device)


def test_the_header_states_the_table():
    text = open(HEADER).read()
    start = text.index("ALIGNMENT AND STRIDES, every entry")
    block = text[start:text.index("*/", start)]
    stated = re.sub(r"\n \*\s+", " ", block)          # the block's lines joined, the comment's margin dropped
    for line in lt.header_lines():
        assert line + " " in stated + " ", f"include/sslam_hip.h does not state: {line}"
    assert len(re.findall(r"\bsslam_\w+: ", stated)) == len(lt.ALIGN), "the header's block has a line the table lacks"


def test_the_sweep_runs_every_row():
    """tests/test_gpu_loose_operands.py has cases, a refusal case and - for an entry with a stride - strided cases for every row of
    the table (its module is importable without a GPU: the cases are built, not run)."""
    import test_gpu_loose_operands as sweep
    assert set(sweep.TABLE) == set(lt.ALIGN), sorted(set(sweep.TABLE) ^ set(lt.ALIGN))
    for entry, r in sweep.TABLE.items():
        assert r["cases"] and r["refuse"] in r["cases"], entry
        assert r["via"] is None or r["via"][0] in lt.ALIGN, entry
    sweep.test_every_entry_with_a_stride_has_strided_rows()
