"""No result may depend on what an uninitialised allocation hands back.  The library takes its outputs, partial tables and
workspaces from torch.empty; a kernel that leaves a tail slab unwritten, or multiplies a stale pad column by a zero weight, is
right on the fresh (mostly zero) memory of a test process and wrong anywhere else.  This module holds

  census()                 every call of an uninitialised allocator in tramba_amd/*.py (an `ast` walk, computed at import);
  poisoned_allocations()   a context in which torch.empty / empty_like / new_empty (and their strided kin) allocate AND FILL:
                           "nan", "zero" or seeded finite "noise" for floating tensors, what CLASSIFICATION allows for integer
                           and byte buffers; every allocation is recorded by the (file, line) of its tramba_amd frame;
  poisoned_numpy()         the same for np.empty (the host tables of hip.py);
  check_independent()      run a case under each fill and once unpatched: finite and bit-identical (or, for the entries that
                           add floats with atomics, each run within the tolerance of its existing test);
  CLASSIFICATION           one row per integer / uint8 device site, from reading the consuming kernels (not from running them);
  EXCLUSIONS               census sites that never hold device memory;
  the stand-ins            plain torch emulations of the four ways a kernel goes wrong here, with an injected fault each
                           (emulation only), for tests/test_buffers_host.py to show that the harness sees them.

The poison may change values, never addresses or trip counts: an integer buffer from which device code forms an address takes
only values that are legal there, and an integer or byte allocation at a tramba_amd site WITHOUT a row raises before anything
runs.  No device code waits on global memory (the scan mailboxes are LDS words polled a bounded number of times,
csrc/ss2d_fused.hip CarryLink::acquire), so no fill can make a launch spin."""
import ast
import contextlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "tramba_amd")
FILLS = ("nan", "zero", "noise")

# ----------------------------------------------------------------------------- census
TORCH_ALLOCATORS = ("empty", "empty_like", "new_empty", "empty_strided", "new_empty_strided", "empty_permuted", "resize_")
LEGACY_TENSORS = ("FloatTensor", "DoubleTensor", "HalfTensor", "BFloat16Tensor", "ByteTensor", "CharTensor", "ShortTensor",
                  "IntTensor", "LongTensor", "BoolTensor")
NUMPY_ROOTS = ("np", "numpy")


def _root_name(node):
    while isinstance(node, ast.Attribute):
        node = node.value
    return node.id if isinstance(node, ast.Name) else None


def census_of_source(src, fname):
    """[(file, line, allocator, kind)] of one source text; kind: "torch", "numpy" (np.empty / np.empty_like) or "legacy"
    (torch.cuda.FloatTensor(n) and its kin).  A line with two calls gives two entries."""
    out = []
    for node in ast.walk(ast.parse(src, fname)):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        name = f.attr if isinstance(f, ast.Attribute) else (f.id if isinstance(f, ast.Name) else None)
        root = _root_name(f.value) if isinstance(f, ast.Attribute) else None
        if name in LEGACY_TENSORS:
            out.append((fname, node.lineno, name, "legacy"))
        elif root in NUMPY_ROOTS and name in ("empty", "empty_like"):
            out.append((fname, node.lineno, name, "numpy"))
        elif name in TORCH_ALLOCATORS:
            out.append((fname, node.lineno, name, "torch"))
    return sorted(out)


def census():
    """every uninitialised allocation of tramba_amd/*.py -> namespace(torch, numpy, legacy: [(file, line, allocator)],
    names: the allocator names in use, by_file: {file: torch sites})"""
    sites = []
    for fname in sorted(os.listdir(PKG)):
        if fname.endswith(".py"):
            with open(os.path.join(PKG, fname)) as fh:
                sites += census_of_source(fh.read(), fname)
    pick = lambda kind: [s[:3] for s in sites if s[3] == kind]
    t = pick("torch")
    by_file = {}
    for s in t:
        by_file[s[0]] = by_file.get(s[0], 0) + 1
    return types.SimpleNamespace(torch=t, numpy=pick("numpy"), legacy=pick("legacy"), names=sorted({s[2] for s in t}),
                                 by_file=by_file)


CENSUS = census()

# ----------------------------------------------------------------------------- the integer and byte sites
# kind "payload": the bytes only ever carry floating-point values (fp32 / fp64 partial sums, saved states): 0xFF bytes.
# kind "integer": integers or pixel bytes that device code reads; `word` is the width they are read in and `values` two
#                 different values that are legal for every such use; `consumer` the device line(s) that read them.
# Made by reading the consumers named, before anything ran on a GPU.
PAYLOAD, INTEGER = "payload", "integer"
CLASSIFICATION = {
    # the (S, S, 4) u8 pixel planes A / T / G of the train transform: every byte is a pixel, and the only table a pixel
    # indexes has 256 entries per channel (the normalisation / label table copied to LDS)
    ("augment.py", "_workspace[key] = torch.empty"): (INTEGER, torch.uint8, (0x00, 0xFF), "csrc/augment.hip:367"),
    # float2 aggregates of the wave-segment scan
    ("hip.py", "ws = _scan_ws[key] = torch.empty"): (PAYLOAD, None, None, "csrc/ss2d_fused.hip:1862"),
    # (B, K, tiles + 8, D) f32 states entering every 32-position tile
    ("hip.py", "return torch.empty(lib().tramba_ss2d_scan_bwd_workspace"): (PAYLOAD, None, None, "csrc/ss2d_fused.hip:1940"),
    ("hip.py", "ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)"): (PAYLOAD, None, None, "csrc/ss2d_fused.hip:1940"),
    # histogram and counts: written by the one kernel (oi[8 + tid] = hist[tid]), read by the host alone
    ("hip.py", "ints = torch.empty((b, EVAL_NINT)"): (INTEGER, torch.int64, (0, 1), "csrc/saliency_eval.hip:198"),
    # pass 1 leaves a mask ROW per pixel (-1: none), pass 2 reads it (arithmetic and a packed site only; the stack index is
    # the column count) and writes the flat index r W + c, from which wfm_tile_kernel forms an address unless it is < 0:
    # -1 is the documented "no feature", 0 a legal row and a legal flat index on every map
    ("hip.py", "idx = torch.empty((b, h, w), dtype=torch.int32"): (INTEGER, torch.int32, (-1, 0), "csrc/saliency_wfm.hip:86 csrc/saliency_wfm.hip:245"),
    # squared distance: a value only (sqrt((double)dist2)), -1 where idx is -1
    ("hip.py", "dist2 = torch.empty_like(idx)"): (INTEGER, torch.int32, (-1, 0), "csrc/saliency_wfm.hip:275"),
    # per-chunk fp32 min / max and per-tile fp64 sums
    ("hip.py", "ws = torch.empty(lib().tramba_weighted_f_workspace"): (PAYLOAD, None, None, "csrc/saliency_wfm.hip:379"),
    # u8 saliency maps: written, then read by the host
    ("hip.py", "out = torch.empty((b, h, w), dtype=torch.uint8"): (INTEGER, torch.uint8, (0x00, 0xFF), "csrc/frames.hip:301"),
    # fp32 partial tables of the attention backward
    ("hip.py", "work = torch.empty(max(nbytes, 16), dtype=torch.uint8"): (PAYLOAD, None, None, "csrc/attention_bwd.hip:613"),
    ("hip.py", "work = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)"): (PAYLOAD, None, None, "csrc/attention_bwd.hip:566"),
    # fp32 partial slabs of the weight-gradient GEMM
    ("hip.py", "ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gy.device)"): (PAYLOAD, None, None, "csrc/train_gemm.hip:621"),
    # ragged u8 maps at the offsets the descriptors name; the bytes between the maps belong to nobody
    ("infer.py", "out = torch.empty(output_bytes(desc), dtype=torch.uint8, device=logits.device)"): (INTEGER, torch.uint8, (0x00, 0xFF), "csrc/frames.hip:339"),
    ("infer.py", "out = torch.empty(output_bytes(desc), dtype=torch.uint8, device=self.device)"): (INTEGER, torch.uint8, (0x00, 0xFF), "csrc/frames.hip:339"),
    ("infer.py", "static_out = torch.empty(cap_out"): (INTEGER, torch.uint8, (0x00, 0xFF), "csrc/frames.hip:339"),
    # the graph's packed input: descriptors, int32 coefficient tables (weights and source indices), frames.  The batch is
    # copied over its head; what stays is past every offset a checked descriptor names.  0 and 1 are legal source indices
    # and legal fixed-point weights should a table word ever be read from there
    ("infer.py", "static_in = torch.empty(cap_in"): (INTEGER, torch.int32, (0, 1), "csrc/frames.hip:250"),
    # inverse permutation of the flattened scan table: inv[flat] = arange writes every entry (flat is a permutation, checked
    # on the line above); read as a row index of a (B, K L, RG) tensor with K L >= 2
    ("modules.py", "inv = torch.empty_like(flat)"): (INTEGER, torch.int64, (0, 1), "modules.py:1174"),
}


# what each consumer line named above says: a kernel edit that moves the code makes tests/test_buffers_host.py fail until the
# row has been read again
CONSUMER_TEXT = {
    "csrc/attention_bwd.hip:566": "static_cast<float *>(work)",
    "csrc/attention_bwd.hip:613": "static_cast<float *>(work)",
    "csrc/augment.hip:367": "lut[i] = tl[kStNorm + i]",
    "csrc/frames.hip:250": "frames_to_input_ragged_kernel",
    "csrc/frames.hip:301": "logits_to_u8_kernel",
    "csrc/frames.hip:339": "logits_to_u8_ragged_kernel",
    "csrc/saliency_eval.hip:198": "oi[8 + tid] = hist[tid]",
    "csrc/saliency_wfm.hip:86": "f[base + j]",
    "csrc/saliency_wfm.hip:245": "p[idx[",
    "csrc/saliency_wfm.hip:275": "sqrt((double)dist2[o])",
    "csrc/saliency_wfm.hip:379": "reinterpret_cast<float *>(workspace)",
    "csrc/ss2d_fused.hip:1862": "reinterpret_cast<float2 *>(workspace)",
    "csrc/ss2d_fused.hip:1940": "(float *)workspace",
    "csrc/train_gemm.hip:621": "(float *)workspace",
    "modules.py:1174": "[:, inv]",
}


def _site_lines():
    """{(file, line): stripped source line} of every torch census site"""
    text = {}
    out = {}
    for f, line, _ in CENSUS.torch:
        if f not in text:
            with open(os.path.join(PKG, f)) as fh:
                text[f] = fh.read().splitlines()
        out[(f, line)] = text[f][line - 1].strip()
    return out


SITE_LINES = _site_lines()


def _resolve(table):
    """rows keyed by (file, a fragment of the source line) -> {(file, line): row}; a fragment must match at least one census
    line of its file (a row that points nowhere is an error), and may match several (the two workspaces of hip._wgrad and
    hip.wgrad_rows_cl are one line of text twice)"""
    out = {}
    for (f, frag), row in table.items():
        hits = [k for k, s in SITE_LINES.items() if k[0] == f and frag in s]
        if not hits:
            raise AssertionError(f"buffer_cases: no allocation in {f} matches {frag!r}")
        for k in hits:
            out[k] = row
    return out


CLASS_BY_SITE = _resolve(CLASSIFICATION)

# census sites that never hold device memory (a 0-dim tensor made to read an element size; a host staging buffer; the host
# branch of DropPath), each with its reason.  At most a tenth of the sites may stand here.
EXCLUSIONS = {
    ("modules.py", "es = torch.empty((), dtype=dtype).element_size()"): "0-dim host tensor, only its element size is read",
    ("train.py", "al = max(1, 16 // torch.empty((), dtype=dtype).element_size())"): "0-dim host tensor, only its element size is read",
    ("parallel.py", "torch.empty((), dtype=self.bucket_dtype).element_size())"): "0-dim host tensor, only its element size is read",
    ("parallel.py", "al = max(1, 16 // torch.empty((), dtype=dtype).element_size())"): "0-dim host tensor, only its element size is read",
    ("infer.py", "buf = torch.empty(at, dtype=torch.uint8, pin_memory=bool(pin))"): "pinned HOST staging buffer of pack_frames",
    ("augment.py", "buf = torch.empty(at, dtype=torch.uint8)"): "HOST staging buffer of augment.pack",
    ("modules.py", "return x.new_empty(shape).bernoulli_(keep).div_(keep)"): "DropPath's branch for HOST tensors (x.is_cuda takes the mask pool); filled by bernoulli_ at once",
}
EXCLUDED_SITES = {k: why for k, why in _resolve(EXCLUSIONS).items()}
MAX_EXCLUSIONS = 13


def device_sites():
    """the (file, line) of every census site that may hold device memory"""
    return sorted({s[:2] for s in CENSUS.torch} - set(EXCLUDED_SITES))


_DTYPE_RE = ("uint8", "int32", "int64", "int16", "int8", "long", "bool")


def integer_sites():
    """device sites whose source line names an integer dtype, plus those the classification lists (an empty_like of an
    integer tensor names no dtype: such a site is found when it first allocates, and raises there without a row)"""
    named = {k for k in device_sites() if any("torch." + d in SITE_LINES[k] for d in _DTYPE_RE)}
    return sorted(named | set(CLASS_BY_SITE))


# ----------------------------------------------------------------------------- the poisoned allocators
PATCHED_TORCH = ("empty", "empty_like", "empty_strided", "empty_permuted")
PATCHED_TENSOR = ("new_empty", "new_empty_strided")
ABSENT = ("resize_",)        # an allocator the harness does not patch: tests/test_buffers_host.py asserts the library has none
NOISE_SEED = 20261019

_active = None


class Poison:
    """the state of one poisoned_allocations() context: .fill, .sites {(file, line): allocations}, .device_sites (those that
    handed out device memory), .unknown (allocations with no tramba_amd frame above them)"""

    def __init__(self, fill):
        self.fill = fill
        self.sites = {}
        self.device_sites = set()
        self.unknown = 0
        self._gen = {}

    def generator(self, device):
        key = str(device)
        g = self._gen.get(key)
        if g is None:
            g = self._gen[key] = torch.Generator(device=device)
            g.manual_seed(NOISE_SEED)
        return g


def _call_site():
    """(file, line) of the nearest frame inside tramba_amd/, or None"""
    f = sys._getframe(2)
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.dirname(os.path.abspath(fn)) == PKG:
            return os.path.basename(fn), f.f_lineno
        f = f.f_back
    return None


def fill_float_(t, fill, gen=None):
    """NaN, zeros, or seeded noise: uniform in (-1, 1), a third of it times 2^12, a third times 2^-12 (finite in fp16 too)"""
    if t.numel() == 0:
        return t
    if fill == "nan":
        return t.fill_(float("nan"))
    if fill == "zero":
        return t.zero_()
    assert fill == "noise", fill
    flat = t.view(-1) if t.is_contiguous() else None
    if t.is_complex():
        return t.fill_(0.5)
    t.uniform_(-1.0, 1.0, generator=gen)
    if flat is not None and flat.numel() >= 3:
        flat[0::3].mul_(4096.0)
        flat[1::3].mul_(1.0 / 4096.0)
    return t


def fill_integer_(t, fill, row):
    """payload rows: 0xFF bytes (zero: 0x00); integer rows: values[0] under "zero", values[1] under "nan" and "noise", as
    words of the row's width (a tail shorter than a word is zeroed)"""
    kind, word, values, _ = row
    if t.numel() == 0:
        return t
    raw = t.view(-1).view(torch.uint8) if t.is_contiguous() else None
    if kind == PAYLOAD:
        assert raw is not None
        return raw.fill_(0x00 if fill == "zero" else 0xFF)
    v = values[0] if fill == "zero" else values[1]
    if t.dtype == word or raw is None:
        return t.fill_(v)
    size = WORD_BYTES[word]
    whole = raw.numel() // size * size
    raw[whole:].zero_()
    if whole:
        raw[:whole].view(word).fill_(v)
    return t


WORD_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}
_active_orig = {}


def _poison_(t, site):
    st = _active
    capturing = t.is_cuda and torch.cuda.is_current_stream_capturing()
    if site is None:
        st.unknown += 1
    else:
        st.sites[site] = st.sites.get(site, 0) + 1
        if t.is_cuda:
            st.device_sites.add(site)
    if capturing or t.layout != torch.strided or t.is_quantized:
        return t              # (a fill under capture would become a node of the graph: the allocation is passed through)
    if t.is_floating_point() or t.is_complex():
        fill_float_(t, st.fill, st.generator(t.device) if st.fill == "noise" else None)
    elif site is not None:
        row = CLASS_BY_SITE.get(site)
        if row is not None:
            fill_integer_(t, st.fill, row)
        elif t.is_cuda:
            raise AssertionError(f"poisoned_allocations: the {t.dtype} device buffer of {site[0]}:{site[1]} has no row in "
                                 f"buffer_cases.CLASSIFICATION (read its consumers, then add one)")
    # an integer tensor allocated outside tramba_amd (the test itself, torch's own Python code) is left as it came
    return t


def _wrap(orig):
    def poisoned(*args, **kwargs):
        t = orig(*args, **kwargs)
        if _active is None or not isinstance(t, torch.Tensor):
            return t
        with torch.no_grad():
            return _poison_(t, _call_site())
    poisoned.__wrapped__ = orig
    return poisoned


@contextlib.contextmanager
def poisoned_allocations(fill):
    """torch.empty, torch.empty_like, torch.Tensor.new_empty and their strided / permuted kin allocate and then fill; the
    originals come back on exit, whatever happens inside.  Yields the Poison record."""
    global _active
    if fill not in FILLS:
        raise ValueError(f"poisoned_allocations: fill {fill!r} is not one of {FILLS}")
    if _active is not None:
        raise RuntimeError("poisoned_allocations does not nest")
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("poisoned_allocations: the current stream is capturing")
    saved = [(torch, n, getattr(torch, n)) for n in PATCHED_TORCH] + [(torch.Tensor, n, getattr(torch.Tensor, n)) for n in PATCHED_TENSOR]
    st = Poison(fill)
    try:
        for owner, n, orig in saved:
            _active_orig[n] = orig
            setattr(owner, n, _wrap(orig))
        _active = st
        yield st
    finally:
        _active = None
        for owner, n, orig in saved:
            setattr(owner, n, orig)
        _active_orig.clear()


def patched_names():
    return set(PATCHED_TORCH) | set(PATCHED_TENSOR)


@contextlib.contextmanager
def poisoned_numpy(byte):
    """np.empty / np.empty_like allocate and then fill every byte with `byte`"""
    saved = (np.empty, np.empty_like)

    def empty(*a, **k):
        out = saved[0](*a, **k)
        out.view(np.uint8).fill(byte) if out.dtype != object and out.flags.c_contiguous else None
        return out

    def empty_like(*a, **k):
        out = saved[1](*a, **k)
        out.view(np.uint8).fill(byte) if out.dtype != object and out.flags.c_contiguous else None
        return out
    try:
        np.empty, np.empty_like = empty, empty_like
        yield
    finally:
        np.empty, np.empty_like = saved


# ----------------------------------------------------------------------------- check_independent
HIT = set()              # device sites that allocated under poison in this process (the coverage gate reads it)


def flatten(res):
    """the tensors of a result, in order: a tensor, None, or nested tuples / lists / dicts of them"""
    if res is None:
        return []
    if isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, dict):
        return [t for k in res for t in flatten(res[k])]
    if isinstance(res, (tuple, list)):
        return [t for r in res for t in flatten(r)]
    raise TypeError(f"check_independent: a result of type {type(res).__name__}")


def _host(ts):
    return [t.detach().cpu().clone() for t in ts]


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def all_finite(t):
    return bool(torch.isfinite(t).all()) if (t.is_floating_point() or t.is_complex()) else True


def check_independent(run, payload=None, exact=True, close=None, fills=FILLS, what=""):
    """run() under every fill and once unpatched.  Every result goes through `payload` (results -> the tensors that carry
    the documented meaningful part; default: every tensor returned).  exact: every run finite and all of them bit-identical.
    Otherwise close(tensors) is called on every run and asserts what the entry's own test asserts against its fp64 oracle;
    every run must still be finite.  Returns the unpatched run's payload (host tensors)."""
    assert exact or close is not None, "a case that is not exact needs the check of its own test"
    payload = payload or flatten
    runs = {}
    for fill in fills:
        with poisoned_allocations(fill) as st:
            res = run()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            runs[fill] = _host(flatten(payload(res)))
        HIT.update(st.device_sites)
    res = run()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    runs["unpatched"] = _host(flatten(payload(res)))
    base = runs["unpatched"]
    assert base, f"{what}: the case returned no tensor"
    for fill, got in runs.items():
        assert len(got) == len(base), f"{what}: {fill} returned {len(got)} tensors, unpatched {len(base)}"
        for i, t in enumerate(got):
            assert all_finite(t), f"{what}: tensor {i} {tuple(t.shape)} is not finite under fill {fill!r}"
        if exact:
            for i, (t, b) in enumerate(zip(got, base)):
                if not same_bits(t, b):
                    d = (t.double() - b.double()).abs()
                    raise AssertionError(f"{what}: tensor {i} {tuple(t.shape)} under fill {fill!r} differs from the unpatched "
                                         f"run in {int((d != 0).sum())} elements (max {float(d.max()):.3e})")
        else:
            close(got)
    return base


# ----------------------------------------------------------------------------- stand-ins (plain torch; faults live here only)
def standin_slab_sum(x, nslab, fault=False):
    """a column sum through a (nslab, n) partial table, the last slab holding the ragged rest; fault: it is never written"""
    m, n = x.shape
    per = (m + nslab - 1) // nslab
    part = torch.empty((nslab, n), dtype=torch.float32)
    for s in range(nslab - 1 if fault else nslab):
        part[s] = x[s * per:(s + 1) * per].sum(0)
    return part.sum(0)


def standin_padded_gemm(x, w, kp, fault=False):
    """y = cols @ wp^T over a column table padded to kp columns, the weight's pad columns zero; fault: the table's pad is left
    as it came (NaN * 0)"""
    m, k = x.shape
    cols = torch.empty((m, kp), dtype=torch.float32)
    cols[:, :k] = x
    if not fault:
        cols[:, k:] = 0
    wp = torch.zeros((w.shape[0], kp), dtype=torch.float32)
    wp[:, :k] = w
    return cols @ wp.t()


def standin_accumulate(x, fault=False):
    """row sums added into a workspace; fault: the workspace is taken for zeros"""
    ws = torch.empty((x.shape[1],), dtype=torch.float32)
    if not fault:
        ws.zero_()
    for row in x:
        ws += row
    return ws


def standin_ragged(x, tile, fault=False):
    """y = 2 x written tile by tile; fault: only whole tiles are written"""
    n = x.numel()
    y = torch.empty_like(x)
    for a in range(0, n - tile + 1 if fault else n, tile):
        y[a:a + tile] = 2 * x[a:a + tile]
    return y


def standin_rows_gemm(x, w, ldy, fault=False):
    """y[:, :n] = x @ w^T into rows of ldy floats: columns n.. are a declared pad nobody writes; fault: column n - 1 is not
    written either"""
    n = w.shape[0]
    y = torch.empty((x.shape[0], ldy), dtype=torch.float32)
    y[:, :n - 1 if fault else n] = (x @ w.t())[:, :n - 1 if fault else n]
    return y


def standin_inputs():
    g = torch.Generator().manual_seed(3)
    return types.SimpleNamespace(x=torch.randn(37, 12, generator=g), w=torch.randn(5, 12, generator=g), v=torch.randn(37, generator=g))


STANDINS = {
    "slab sum, last slab unwritten": lambda s, fault: standin_slab_sum(s.x, 4, fault),
    "padded column table times zero weights": lambda s, fault: standin_padded_gemm(s.x, s.w, 16, fault),
    "accumulation into a workspace taken for zeros": lambda s, fault: standin_accumulate(s.x, fault),
    "ragged tile, whole tiles only": lambda s, fault: standin_ragged(s.v, 8, fault),
}
