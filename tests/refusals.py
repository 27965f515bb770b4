"""The one harness of the host tests' refusals.

The library refuses a bad call on the host, before its first HIP call.  The host tests hold it to that with made-up
device addresses (256-byte aligned, never dereferenced), and an address stays undereferenced only while the refusal under
test is still there.  So every such call is made here, in a child process that sees no device (HIP_VISIBLE_DEVICES and
ROCR_VISIBLE_DEVICES empty): a call the library failed to refuse fails at its first HIP call, comes back as MVS_ERR_HIP
(4) and is reported as "reached a HIP call" instead of reaching hardware.  No test process passes a made-up address to
an entry point itself.

A host module states its cases in a table REFUSALS = {entry point: spec} (or a function of the child's `part` that
returns one).  A spec is a dict:
    good:     value of every argument by parameter name, the base every case overrides; a callable is given the
              overridden arguments (a count that follows an array's length); a workspace_bytes that is left out is ample
    host:     the pointer parameters that are real host memory -> their element ctype (the array is built from the
              argument's sequence) or a callable (arguments, overrides) -> ctypes object; a `size_t*` needs no entry
    sizes:    name -> callable(arguments) for byte counts: an integer argument overridden with "need" or "need-1" (or
              any other name here, "-1" likewise) gets that count
    optional: the pointers that may be NULL (read by the completeness test of tests/test_abi_domain_host.py)
    extra:    names a case may override that are neither a parameter nor in `good` (read by a `host` callable)
    cases:    [(label, overrides by parameter name, expected status, fragment of the message)]
A pointer is overridden with None (NULL) or "plus4", "plus16", ... (its made-up address moved off its alignment).

The child, `python tests/refusals.py MODULE [part]`, imports MODULE and runs every case of its table: a refusal nobody
else makes first sets the thread's error string, so that a refusal without its own message shows as `stale`; an "about to
call" record is printed and flushed before the call, so that a process death is pinned on its case; the call is built
from the header's prototype by parameter name; the result record replaces the first.  A module's
refusals_epilogue(lib), if it has one, runs after the sweep.
"""
import ctypes
import glob
import importlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _path in (REPO, HERE):
    if _path not in sys.path:
        sys.path.insert(0, _path)

OK, BAD_SHAPE, BAD_DTYPE, WORKSPACE, HIP, NULL = 0, 1, 2, 3, 4, 5
NAN, INF = float("nan"), float("inf")
BIN = ((-305.0, -205.0, -20.0), (305.0, 205.0, 220.0))
AMPLE = 1 << 44         # a workspace_bytes no case is short of
BOX = dict(box_min=ctypes.c_double, box_max=ctypes.c_double)      # the `host` entries of a cloud entry point's box
HEADERS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(REPO, "include", "*.h")))
_C_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
              "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}


def fake(k, off=0):
    """The k-th made-up device address: 256-byte aligned, never dereferenced."""
    return ctypes.c_void_p(0x100000 * k + off)


def header_text(header):
    return open(os.path.join(REPO, "include", header)).read()


def declarations(header):
    """[(entry point, [(C type without const, parameter name)])] in the header's order.  Comments inside a prototype are
    dropped and `double box_min[3]` is read as `double* box_min`, which is the same C parameter."""
    src = re.sub(r"/\*.*?\*/", " ", header_text(header), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"(\w+)\s*\[\s*\d+\s*\]", r"* \1", src)
    out = []
    for name, params in re.findall(r"^(?:int|const char\*)\s+(mvs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        plist = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            ctype = re.sub(r"\bconst\b", " ", re.sub(r"\w+\s*$", "", param.strip())).replace("*", " * ")
            plist.append((" ".join(ctype.split()), re.search(r"(\w+)\s*$", param).group(1)))
        out.append((name, plist))
    return out


def prototypes(header):
    """{entry point: [(kind, name)]}; kind is 'ptr' or the scalar's C type."""
    return {name: [("ptr" if "*" in c else c, p) for c, p in plist] for name, plist in declarations(header)}


def all_prototypes():
    return {name: plist for h in HEADERS for name, plist in prototypes(h).items()}


def header_argtypes(header):
    """{entry point: the ctypes argument list its prototype asks for}: `size_t*` is POINTER(c_size_t), a pointer to
    pointers (`const float* const*`) POINTER(c_void_p), any other pointer c_void_p, a scalar its ctype."""
    def kind(c):
        return ctypes.POINTER(ctypes.c_void_p) if c.count("*") == 2 else ctypes.POINTER(ctypes.c_size_t) if c == "size_t *" \
            else ctypes.c_void_p if c.endswith("*") else _C_SCALARS[c]
    return {name: [kind(c) for c, _ in plist] for name, plist in declarations(header)}


def label(ov):
    """The label of a case that is named by its overrides."""
    return ", ".join(f"{k}={v}" for k, v in ov.items()) or "good"


def cases(*rows):
    """[(overrides, status, fragment)] -> cases labelled by their overrides; an exact duplicate is kept once."""
    out = {}
    for ov, want, text in rows:
        assert out.setdefault(label(ov), (label(ov), ov, want, text))[2:] == (want, text), ov
    return list(out.values())


def table_of(module, part=None):
    table = module.REFUSALS
    return table(part) if callable(table) else table


# ---- the child ----------------------------------------------------------------------------------------------------------
def call(lib, protos, name, spec, ov):
    """One call of `name`, built from its prototype: the good arguments, `ov` over them."""
    a = dict(spec.get("good", {}))
    unknown = set(ov) - set(a) - {p for _, p in protos[name]} - set(spec.get("extra", ()))
    assert not unknown, (name, unknown)
    host, sizes = spec.get("host", {}), spec.get("sizes", {})
    a.update({k: v for k, v in ov.items() if not (v is None and k in host)})      # a NULL array keeps its good length
    a = {k: v(a) if callable(v) else v for k, v in a.items()}
    args, keep, k = [], [], 0
    for kind, p in protos[name]:
        if kind == "ptr":
            k += 1
            if p == "stream" or (ov[p] if p in ov else a.get(p, 0)) is None:      # NULL by the case, or in the good call
                v = None
            elif p in host:
                v = (host[p] * max(len(a[p]), 1))(*a[p]) if hasattr(host[p], "_type_") else host[p](a, ov)
                keep.append(v)
            elif p == "bytes":
                keep.append(ctypes.c_size_t(0))
                v = ctypes.byref(keep[-1])
            else:
                v = fake(k, int(ov[p][len("plus"):]) if p in ov else 0)
        else:
            v = a.get(p, AMPLE if p == "workspace_bytes" else None)
            if isinstance(v, str):
                v = sizes[v[:-2]](a) - 1 if v.endswith("-1") else sizes[v](a)
            assert v is not None, (name, p)
        args.append(v)
    st = getattr(lib, name)(*args)
    return st, (lib.mvs_last_error_string() or b"").decode("utf-8", "replace")


def child(module, part=None):
    from scene_3dreconstruction_mvsnet_amd import _lib
    lib = _lib.load()
    protos = all_prototypes()

    def sentinel():
        assert lib.mvs_query_feature_workspace(1, 3, 2, ctypes.byref(ctypes.c_size_t(0))) == BAD_SHAPE
        return lib.mvs_last_error_string().decode("utf-8", "replace")
    mod = importlib.import_module(module)
    for name, spec in table_of(mod, part).items():
        for lab, ov, want, _ in spec["cases"]:
            before = sentinel()
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=None, err="")), flush=True)      # about to call
            got, err = call(lib, protos, name, spec, ov)
            print("R " + json.dumps(dict(ep=name, case=lab, want=want, got=got, err=err, stale=err == before)), flush=True)
    if hasattr(mod, "refusals_epilogue"):
        mod.refusals_epilogue(lib)


# ---- the parent ---------------------------------------------------------------------------------------------------------
_records = {}       # run: key -> (Child, records)


def run(module, part=None, env=None):
    """The child of `module` (a host test module's __name__), run once per (module, part, env) -> (gpu_child.Child,
    {(entry point, label): its last record})."""
    import gpu_child
    module = module.rpartition(".")[2]
    argv = ["refusals.py", module] + ([part] if part else [])
    key = ("refusals", module, part, tuple(sorted((env or {}).items())))
    if key not in _records:
        r = gpu_child.run_once(key, argv, timeout=300, gpu=False, env=env)
        # the record after a call replaces the one before it
        _records[key] = r, {(rec["ep"], rec["case"]): rec for rec in r.records("R ")}
    return _records[key]


def wrong(rec, want, text=""):
    """What is wrong with a case's record, or None: the status is the expected one and, for a refusal, the message is
    this refusal's own (not the one a refusal before it left) and holds the fragment."""
    if rec is None:
        return "the child never came to this call"
    if rec["got"] != want:
        what = "the process died in this call" if rec["got"] is None else \
            "reached a HIP call" if rec["got"] == HIP else f"returned {rec['got']}"
        return f"{what}, expected {want} ({rec['err']})"
    if want not in (OK, HIP) and (rec["stale"] or not rec["err"].strip() or text not in rec["err"]):
        return f"status {want} without its message {text!r}: {rec['err']!r}{' (stale)' if rec['stale'] else ''}"
    return None


def check(module, names=None, part=None, env=None):
    """Every case of `module`'s table (of the entry points `names`) against the child's records."""
    r, records = run(module.__name__, part, env)
    bad, n = [], 0
    for name, spec in table_of(module, part).items():
        if names is None or name in names:
            labels = [c[0] for c in spec["cases"]]
            assert len(set(labels)) == len(labels), name
            for lab, _, want, text in spec["cases"]:
                n += 1
                why = wrong(records.get((name, lab)), want, text)
                if why:
                    bad.append(f"{name}: {lab}: {why}")
    assert not bad, f"{len(bad)} of {n} cases:\n" + "\n".join(bad)
    assert r.returncode == 0, f"the child ended with status {r.returncode}:\n{r.stderr[-2000:]}"
    return n


def expect(module, name, ov=None, **kw):
    """One case of `module`'s table, found by its overrides, against its record."""
    ov = dict(ov or {}, **kw)
    found = [c for c in table_of(module)[name]["cases"] if c[0] == label(ov)]
    assert len(found) == 1, (name, label(ov))
    _, _, want, text = found[0]
    why = wrong(run(module.__name__)[1].get((name, found[0][0])), want, text)
    assert not why, f"{name}: {found[0][0]}: {why}"
    return want


# ---- a header's declarations --------------------------------------------------------------------------------------------
def check_header(header, symbols):
    """What holds for every header of include/: its declared names, in order, are the Python layer's table and its
    *_SYMBOLS tuple; no other header's table or text has them; the argument kinds are the prototypes' and the loaded
    library's; the raw library exports them; the table's keys are the headers present.  -> the header's text"""
    from scene_3dreconstruction_mvsnet_amd import _lib
    declared = [name for name, _ in declarations(header)]
    assert declared == list(_lib._ABI[header]) == list(symbols) and len(set(declared)) == len(declared)
    assert sorted(_lib._ABI) == HEADERS
    for other in HEADERS:
        if other != header:
            assert not set(declared) & set(_lib._ABI[other]), other
            assert not set(declared) & {name for name, _ in declarations(other)}, other
    kinds = header_argtypes(header)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert _lib._ABI[header][name] == kinds[name], name
        assert list(getattr(_lib.load(), name).argtypes) == kinds[name], name
        assert hasattr(raw, name), name
    return header_text(header)


def define(src, name):
    return int(re.search(rf"^#define {name} (\d+)", src, flags=re.M).group(1))


if __name__ == "__main__":
    child(*sys.argv[1:3])
