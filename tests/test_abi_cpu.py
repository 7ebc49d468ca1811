"""CPU checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/mmidx.h declares, and fails loudly (never falls back) without a GPU."""
import ctypes as C
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    m.build()
    return m


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mmidx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mmidx_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_exported(mi):
    L = mi.lib()
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/mmidx.h but not exported"
    # and the python binding covers every one of them
    from importlib import import_module
    nat = import_module("multimedia-indexing_amd._native")
    assert sorted(nat.SIGNATURES) == names
    assert L.mmidx_abi_version() == 8


def test_argument_errors_without_touching_the_gpu(mi):
    L = mi.lib()
    h = C.c_void_p()
    # IVFPQ.java:181-183 / PQ.java:148-150
    st = L.mmidx_create(2, 10, 3, 256, 16, 0, None, None, 0, C.byref(h))
    assert st == 1 and b"subvectors is not valid" in L.mmidx_last_error()
    assert L.mmidx_create(7, 8, 2, 256, 16, 0, None, None, 0, C.byref(h)) == 6
    assert L.mmidx_create(2, 8, 2, 256, 16, 1, None, None, 0, C.byref(h)) == 6  # rotation w/o matrix
    assert L.mmidx_create(2, 8, 2, 256, 16, 0, None, None, 0, None) == 6
    assert L.mmidx_set_w(None, 3) == 6
    assert L.mmidx_destroy(None) == 0
    # k-means: point indices, hipcub's item counts and the JDK draws are 32-bit -- n >= 2^31 is refused before any device
    # call (dummy non-null buffers: nothing may be read or written through them)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        assert L.mmidx_kmeans_device(0, n, 8, 16, 4, 1, 1, p, None, p, None, None, None, None, None) == 6
        assert L.mmidx_kmeans(0, n, 8, 16, 4, 1, 0, p, None, p, None, None, None, None) == 6
    assert L.mmidx_kmeans_device(0, 8, 2, 9, 4, 1, 0, p, None, p, None, None, None, None, None) == 6  # k > n
    assert all(v == 0.0 for v in buf)


@pytest.mark.skipif(importlib.import_module("multimedia-indexing_amd").lib().mmidx_device_count() > 0,
                    reason="a GPU is present")
def test_no_cpu_fallback(mi):
    """Without a HIP device the product path must fail, not silently compute on the host."""
    with pytest.raises(mi.MmidxError) as ei:
        mi.IVFPQ(8, 100, False, "", 2, 4, 0, 4, 512)
    assert ei.value.status == 8
    with pytest.raises(mi.MmidxError):
        mi.PQ(8, 100, False, "", 2, 4, 0, 512)


def test_product_does_not_reference_the_oracle():
    """The shipped path must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "multimedia-indexing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "mmidx_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def _read(*parts):
    return open(os.path.join(ROOT, *parts), errors="replace").read()


def option_table_names():
    """the names in the rows of kOptions (csrc/mmidx_api.hip)"""
    src = _read("multimedia-indexing_amd", "csrc", "mmidx_api.hip")
    table = src[src.index("const OptionRow kOptions[] = {"):]
    return re.findall(r'^    \{"(\w+)",', table[:table.index("\n};")], flags=re.M)


def test_option_table_matches_header_and_callers():
    """The switch surface is one table: include/mmidx.h lists exactly its names, every caller in the tree passes a name that
    exists, and nothing of the retired switches is left in the product."""
    names = option_table_names()
    assert len(names) >= 30 and len(set(names)) == len(names)
    # (a) the header's list: the lines `"name": text` between the list's opening sentence and the sharded handle's own options
    hdr = _read("include", "mmidx.h")
    lst = hdr[hdr.index("/* Runtime switches for measurements and tests"):hdr.index("int mmidx_set_option(")]
    own, shard = lst.split(" * A sharded handle passes these on")
    assert sorted(re.findall(r'^ \*   "(\w+)":', own, flags=re.M)) == sorted(names)
    # ... and the group-level ones are those of sharded_set_option
    sh = _read("multimedia-indexing_amd", "csrc", "mmidx_sharded.h")
    sh = sh[sh.index("int sharded_set_option("):]
    shard_names = set(re.findall(r'n == "(\w+)"', sh[:sh.index("\n}\n")]))
    assert set(re.findall(r'^ \*   "(\w+)":', shard, flags=re.M)) == shard_names and len(shard_names) == 6
    # (b) every literal option name a caller passes is known.  The VLAD and bag-of-words aggregators have set_option entry
    # points of their own (mmidx_vlad_set_option, mmidx_bow_set_option): their names are read from the sources the same way;
    # "no_such_option" is what tests pass to see the refusal.
    api = _read("multimedia-indexing_amd", "csrc", "mmidx_api.hip")
    vlad = _read("multimedia-indexing_amd", "csrc", "mmidx_frontend.hip")
    vlad = vlad[vlad.index("int mmidx_vlad_set_option("):]
    aggregator = set(re.findall(r'== "(\w+)"', vlad[:vlad.index("\n}\n")] + _read("multimedia-indexing_amd", "csrc", "mmidx_bow.hip")))
    known = set(names) | shard_names | aggregator | {"no_such_option"}
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "multimedia-indexing_amd", "csrc", "mmidx_bow.hip")]
    for top in ("tests", "tools", "examples", "multimedia-indexing_amd"):
        for dirpath, dirs, fs in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if not (top == "tools" and d == "dbg") and d != "__pycache__"]
            files += [os.path.join(dirpath, f) for f in fs if f.endswith((".py", ".java", ".c"))]
    seen = set()
    for f in files:
        for n in re.findall(r'set_option\(\s*(?:[\w.>\-]+\s*,\s*)?b?["\'](\w+)["\']', open(f, errors="replace").read()):
            assert n in known, f"{f} passes option '{n}', which no set_option knows"
            seen.add(n)
    assert {"exhaustive", "exact_coarse", "passa_q", "tie_slots"} <= seen  # (the scan does find the callers)
    # (c) the retired switches and the code only they reached are gone from the product
    retired = ["k_scan_seed", "launch_scan_seeded", "passa_512", "passa_su2", "passa_filter", "passa_prefix", "no_seed", "code_lo", "code_hi",
               "coarse_nodma", "no_item_compaction", "grp_blocks", "MMIDX_ASSIGN_SPLIT", "MMIDX_VLAD_EXACT"]
    for top in ("multimedia-indexing_amd", "include"):
        for dirpath, dirs, fs in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d != "__pycache__"]
            for f in fs:
                if f.endswith((".so", ".o", ".pyc")):
                    continue
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                for r in retired:
                    assert not re.search(r"\b" + r + r"\b", txt), f"{os.path.join(dirpath, f)} still names {r}"
    assert '"lut_pre"' not in api  # (the ScanParams field and the kernel keep the name; only the option went)
