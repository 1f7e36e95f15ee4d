"""CPU side of the uninitialised-memory harness (tests/golden/buffer_cases.py): the fills are what they claim and the patched
allocators come back whatever happens; every allocator form the library uses is one the harness patches; plain torch stand-ins
of the four ways a kernel goes wrong on stale memory -- each with an injected fault, in the emulation only, never in a kernel
-- are caught and their correct versions pass; the classification covers every integer and byte site of the census and points
at lines that exist; and the host tables hip.py takes from np.empty do not depend on what np.empty hands back."""
import os

import numpy as np
import pytest
import torch

import buffer_cases as bc
from tramba_amd import data, hip

PKG = bc.PKG


# ----------------------------------------------------------------------------- fills and restoration
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
def test_float_fills(dtype):
    with bc.poisoned_allocations("nan"):
        t = torch.empty((5, 7), dtype=dtype)
        u = torch.empty_like(t)
        v = t.new_empty((3,))
        s = torch.empty_strided((4, 3), (1, 4), dtype=dtype)
    for x in (t, u, v, s):
        assert x.dtype == dtype and bool(torch.isnan(x).all())
    with bc.poisoned_allocations("zero"):
        t = torch.empty((5, 7), dtype=dtype)
    assert bool((t == 0).all())
    with bc.poisoned_allocations("noise"):
        a = torch.empty((999,), dtype=dtype)
        b = torch.empty((999,), dtype=dtype)
    with bc.poisoned_allocations("noise"):
        a2 = torch.empty((999,), dtype=dtype)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, a2) and not torch.equal(a, b)          # seeded per context
    mag = a.double().abs()
    assert float(mag.max()) > 64 and float(mag[mag > 0].min()) < 2.0 ** -12 and float(mag.max()) <= 4096.0
    assert len(set(a.tolist())) > 500


def test_integer_fills_follow_the_row():
    pay = (bc.PAYLOAD, None, None, "x:1")
    t = torch.zeros(16, dtype=torch.uint8)
    assert bool((bc.fill_integer_(t, "nan", pay) == 0xFF).all()) and bool((bc.fill_integer_(t, "noise", pay) == 0xFF).all())
    assert bool((bc.fill_integer_(t, "zero", pay) == 0).all())
    assert bool(torch.isnan(bc.fill_integer_(torch.zeros(16, dtype=torch.uint8), "nan", pay).view(torch.float32)).all())
    row = (bc.INTEGER, torch.int32, (-1, 0), "x:1")
    i = torch.full((6,), 7, dtype=torch.int32)
    assert bc.fill_integer_(i, "zero", row).tolist() == [-1] * 6 and bc.fill_integer_(i, "nan", row).tolist() == [0] * 6
    words = (bc.INTEGER, torch.int32, (0, 1), "x:1")
    raw = torch.full((11,), 9, dtype=torch.uint8)                       # two whole words and a tail of three bytes
    bc.fill_integer_(raw, "noise", words)
    assert raw[:8].view(torch.int32).tolist() == [1, 1] and raw[8:].tolist() == [0, 0, 0]
    for kind, word, values, _ in bc.CLASSIFICATION.values():
        assert kind in (bc.PAYLOAD, bc.INTEGER)
        if kind == bc.INTEGER:
            assert word in bc.WORD_BYTES and len(values) == 2 and values[0] != values[1]


def test_integer_tensors_outside_the_library_are_left_alone():
    with bc.poisoned_allocations("nan") as st:
        t = torch.empty((4,), dtype=torch.int64)
        f = torch.empty((4,))
    assert st.unknown == 2 and st.sites == {} and bool(torch.isnan(f).all()) and t.dtype == torch.int64


def test_originals_come_back_after_an_exception_and_nesting_is_refused():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, torch.Tensor.new_empty_strided)
    with pytest.raises(KeyError):
        with bc.poisoned_allocations("nan"):
            assert torch.empty is not before[0]
            raise KeyError("inside")
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, torch.Tensor.new_empty_strided)
    assert all(a is b for a, b in zip(before, after))
    with bc.poisoned_allocations("zero"):
        with pytest.raises(RuntimeError, match="nest"):
            with bc.poisoned_allocations("nan"):
                pass
        assert bool((torch.empty(3) == 0).all())               # the outer context is still the one in force
    assert torch.empty is before[0]
    with pytest.raises(ValueError):
        with bc.poisoned_allocations("ones"):
            pass
    with bc.poisoned_allocations("nan"):                       # and a refused fill leaves nothing behind
        pass
    assert torch.empty is before[0]
    e, el = np.empty, np.empty_like
    with pytest.raises(KeyError):
        with bc.poisoned_numpy(0xA5):
            assert int(np.empty(3, np.int32)[0]) == int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
            raise KeyError("inside")
    assert np.empty is e and np.empty_like is el


def test_call_sites_are_those_of_the_library():
    """an allocation is recorded under the (file, line) of the nearest frame whose code lives in tramba_amd/"""
    with bc.poisoned_allocations("nan") as st:
        hip_like = os.path.join(PKG, "hip.py")
        code = compile("import torch\ndef f():\n    return torch.empty(3)\n", hip_like, "exec")
        ns = {}
        exec(code, ns)
        t = ns["f"]()
    assert st.sites == {("hip.py", 3): 1} and st.device_sites == set() and bool(torch.isnan(t).all())


# ----------------------------------------------------------------------------- patch completeness
def test_every_allocator_form_of_the_library_is_patched_or_absent():
    c = bc.CENSUS
    assert c.torch and c.numpy
    for name in c.names:
        assert name in bc.patched_names(), f"tramba_amd uses {name}: poisoned_allocations does not patch it"
    for name in bc.ABSENT:
        assert name not in c.names
    assert c.legacy == [], c.legacy
    assert set(bc.TORCH_ALLOCATORS) == bc.patched_names() | set(bc.ABSENT)
    assert {s[2] for s in c.numpy} <= {"empty", "empty_like"}


def test_census_sees_every_form():
    src = ("import torch, numpy as np\n"
           "a = torch.empty(3)\n"
           "b = torch.empty_like(a); c = a.new_empty(2)\n"
           "d = torch.empty_strided((2,), (1,))\n"
           "e = a.new_empty_strided((2,), (1,))\n"
           "f = torch.empty_permuted((2, 3), (1, 0))\n"
           "a.resize_(9)\n"
           "g = np.empty(4)\n"
           "h = torch.cuda.FloatTensor(5)\n"
           "i = torch.zeros(3)\n")
    got = bc.census_of_source(src, "x.py")
    assert [(s[1], s[2], s[3]) for s in got] == [(2, "empty", "torch"), (3, "empty_like", "torch"), (3, "new_empty", "torch"),
                                                 (4, "empty_strided", "torch"), (5, "new_empty_strided", "torch"),
                                                 (6, "empty_permuted", "torch"), (7, "resize_", "torch"), (8, "empty", "numpy"),
                                                 (9, "FloatTensor", "legacy")]
    assert sum(bc.CENSUS.by_file.values()) == len(bc.CENSUS.torch)
    assert set(bc.CENSUS.by_file) >= {"hip.py", "modules.py", "infer.py", "train.py", "augment.py", "parallel.py"}
    assert {s[0] for s in bc.CENSUS.numpy} == {"hip.py"} and len(bc.CENSUS.numpy) == 7


# ----------------------------------------------------------------------------- the harness sees what it is for
@pytest.mark.parametrize("name", list(bc.STANDINS))
def test_injected_faults_are_caught_and_correct_versions_pass(name):
    s = bc.standin_inputs()
    fn = bc.STANDINS[name]
    bc.check_independent(lambda: fn(s, False), what=name)
    with pytest.raises(AssertionError):
        bc.check_independent(lambda: fn(s, True), what=name)
    # the fault is invisible on zeroed memory alone where the buggy code happens to be right there, and visible to NaN
    with bc.poisoned_allocations("nan"):
        assert not bool(torch.isfinite(fn(s, True)).all())
        assert bool(torch.isfinite(fn(s, False)).all())


def test_zero_fill_alone_would_miss_the_zero_assuming_faults():
    """what a fresh process does: the two faults that ASSUME zeros are exactly right on zeroed memory"""
    s = bc.standin_inputs()
    for name in ("padded column table times zero weights", "accumulation into a workspace taken for zeros"):
        with bc.poisoned_allocations("zero"):
            bad = bc.STANDINS[name](s, True)
        good = bc.STANDINS[name](s, False)
        assert torch.equal(bad, good), name


def test_payload_hides_a_declared_pad_and_nothing_else():
    s = bc.standin_inputs()
    n = s.w.shape[0]
    run = lambda fault: (lambda: bc.standin_rows_gemm(s.x, s.w, 8, fault))
    with pytest.raises(AssertionError):
        bc.check_independent(run(False), what="rows_gemm, whole rows")                       # the pad is nobody's
    bc.check_independent(run(False), payload=lambda y: y[:, :n], what="rows_gemm, columns :n")
    with pytest.raises(AssertionError):
        bc.check_independent(run(True), payload=lambda y: y[:, :n], what="rows_gemm, a payload column unwritten")


def test_tolerance_mode_still_asks_for_finite_runs():
    s = bc.standin_inputs()
    want = s.x.double().sum(0)

    def close(ts):
        assert float((ts[0].double() - want).abs().max()) <= 1e-5
    bc.check_independent(lambda: bc.standin_accumulate(s.x), exact=False, close=close)
    with pytest.raises(AssertionError):
        bc.check_independent(lambda: bc.standin_accumulate(s.x, True), exact=False, close=close)
    with pytest.raises(AssertionError):
        bc.check_independent(lambda: bc.standin_accumulate(s.x), exact=False)                # no check named


# ----------------------------------------------------------------------------- classification and exclusions
def test_classification_covers_every_integer_site_and_points_at_real_lines():
    sites = set(bc.device_sites())
    for site in bc.integer_sites():
        assert site in bc.CLASS_BY_SITE, f"{site[0]}:{site[1]} ({bc.SITE_LINES[site]}) has no classification row"
    for site, (kind, word, values, consumer) in bc.CLASS_BY_SITE.items():
        assert site in sites, site
        assert consumer, site
        for ref in consumer.split():
            path, line = ref.rsplit(":", 1)
            full = os.path.join(PKG, path)
            assert os.path.exists(full), ref
            with open(full) as fh:
                lines = fh.read().splitlines()
            assert 1 <= int(line) <= len(lines), ref
            assert ref in bc.CONSUMER_TEXT and bc.CONSUMER_TEXT[ref] in lines[int(line) - 1], \
                f"{ref} no longer reads {bc.CONSUMER_TEXT.get(ref)!r}: read the consumer again and update the row"
    # the rows the census can find by dtype: every uint8 / int32 / int64 buffer that may live on the device
    assert len([s for s in bc.integer_sites()]) >= 17


def test_exclusions_are_few_reasoned_and_hold_no_device_memory():
    assert 0 < len(bc.EXCLUDED_SITES) <= bc.MAX_EXCLUSIONS
    assert len(bc.EXCLUDED_SITES) * 10 <= len(bc.CENSUS.torch)
    for site, why in bc.EXCLUDED_SITES.items():
        assert why and len(why) > 10
        line = bc.SITE_LINES[site]
        assert "device=" not in line, (site, line)                # nothing here is placed on a device
    assert not set(bc.EXCLUDED_SITES) & set(bc.CLASS_BY_SITE)


# ----------------------------------------------------------------------------- host tables
def _tables_under(byte):
    out = {}
    with bc.poisoned_numpy(byte):
        for fam in hip.FAMILY:
            for h in (5, 12, 16):
                t = hip.scan_table_host(fam, h, h, hip.default_window(h) if fam in ("window", "dilation") else 0)
                ptr, idx = hip.scan_table_inverse_host(t)
                out[("scan", fam, h)] = (t, ptr, idx)
        out["resize"] = (hip.resize_table_host(1, 1, 1, 1, data.IMAGENET_MEAN, data.IMAGENET_STD),
                         hip.resize_table_host(2, 3, 1, 2, data.IMAGENET_MEAN, data.IMAGENET_STD))
        out["aug_source"] = (hip.augment_source_table_host(1, 1, 3), hip.augment_source_table_host(2, 5, 3))
        out["aug_size"] = (hip.augment_size_table_host(3, data.IMAGENET_MEAN, data.IMAGENET_STD),)
        out["aug_rot"] = (hip.augment_rotation(3, 1), hip.augment_rotation(3, 359))
    return out


def test_host_tables_do_not_depend_on_what_np_empty_hands_back():
    """the 7 np.empty sites of hip.py are filled by host C functions: identical under two fills (a word left unwritten would
    hold 0x00000000 in one run and 0xA5A5A5A5 in the other)"""
    a, b = _tables_under(0x00), _tables_under(0xA5)
    assert a.keys() == b.keys() and len(a) == 3 * len(hip.FAMILY) + 4
    for key in a:
        for x, y in zip(a[key], b[key]):
            assert x.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), key
    with bc.poisoned_numpy(0xA5):
        assert int(np.empty(2, np.int32)[1]) == int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
