"""Which kernel served a launch: a recorder for the exact contraction tests (no test inside).

`recording(tmp_dir)` opens a profiling window with the filter cleared and yields a list that, once the window is
closed, holds one (kernel name, description) per contraction launch made inside it. The library writes one line per
recorded launch -- kind, description (cn_prof_desc), microseconds, flops, kernel name (cn_prof_name) -- to the file
CN_PROF_DUMP names when the window closes; the variable is set in-process for the window only and restored afterwards.
The names are cross-checked against cn_profile_top (the per-name aggregates bench.py reads).

`route_key(name, desc)` keeps the facts of a launch that select a code path and drops the sizes. `Routes` collects the
keys a test emits, part by part, and compares them with the test's entry in tests/contraction_routes.py.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re
import shutil
import subprocess
import typing as T

FAMILIES = ("cn_conv_igemm_vec_kernel", "cn_conv_igemm_kernel", "cn_wgrad_vec_kernel", "cn_wgrad_vec3_kernel",
            "cn_wgrad_kernel", "cn_bconv_kernel", "cn_bwgrad_kernel", "cn_gemm1x1_kernel", "cn_pretime_kernel")


def _lib():
    from cultionet_amd import _lib

    return _lib


def profile_top():
    """[(kernel name, launches)] of the window just closed, from cn_profile_top."""
    L = _lib()
    nb, o3 = ctypes.create_string_buffer(96), (ctypes.c_double * 3)()
    out = []
    for r in range(L.query("cn_profile_top", 0, nb, 96, o3)):
        L.query("cn_profile_top", r, nb, 96, o3)
        out.append((nb.value.decode(), int(o3[2])))
    return out


@contextlib.contextmanager
def recording(tmp_dir):
    """Yields a list; after the block it holds (name, desc) of every contraction launch made inside, in launch order."""
    import torch

    L = _lib()
    dump = os.path.join(str(tmp_dir), "cn_prof_dump.tsv")
    if os.path.exists(dump):
        os.remove(dump)
    launches: T.List[T.Tuple[str, str]] = []
    torch.cuda.synchronize()
    old = os.environ.get("CN_PROF_DUMP")
    os.environ["CN_PROF_DUMP"] = dump
    L.call("cn_profile_set_filter", None)
    L.call("cn_profile_begin")
    try:
        yield launches
        torch.cuda.synchronize()
    finally:
        try:
            L.call("cn_profile_end", (ctypes.c_double * 24)())
        finally:
            if old is None:
                os.environ.pop("CN_PROF_DUMP", None)
            else:
                os.environ["CN_PROF_DUMP"] = old
    if os.path.exists(dump):
        with open(dump) as f:
            for line in f:
                cols = line.rstrip("\n").split("\t")
                assert len(cols) == 5, f"CN_PROF_DUMP line without a kernel name: {line!r}"
                launches.append((cols[4], cols[1]))
        os.remove(dump)
    counts: T.Dict[str, int] = {}
    for name, _ in launches:
        counts[name] = counts.get(name, 0) + 1
    assert counts == dict(profile_top()), f"dump file and cn_profile_top disagree: {counts} vs {profile_top()}"


def _num(desc, tag, default=None):
    m = re.search(r"(?:^| )" + re.escape(tag) + r"(-?\d+)(?= |$|/|x)", desc)
    if m is None:
        assert default is not None, f"launch description without {tag!r}: {desc!r}"
        return default
    return int(m.group(1))


def _splits(desc):
    m = re.search(r" grid\d+x\d+x(\d+)(?= |$)", desc)
    assert m, f"launch description without a grid: {desc!r}"
    return int(m.group(1))


def route_key(name: str, desc: str) -> T.Tuple[str, ...]:
    """The facts of one recorded launch that select a code path (sizes dropped), as a tuple of strings."""
    fam = name.split("<")[0]
    if fam in ("cn_conv_igemm_vec_kernel", "cn_conv_igemm_kernel"):
        return (name, "G>1" if _num(desc, "G") > 1 else "G1", f"cls{_num(desc, 'cls')}", f"is{_num(desc, 'is')}",
                f"os{_num(desc, 'os')}", f"taps{_num(desc, 'taps')}", "split" if _splits(desc) > 1 else "whole",
                f"il{_num(desc, 'il')}")
    if fam in ("cn_wgrad_vec_kernel", "cn_wgrad_vec3_kernel"):
        return (name, f"G{_num(desc, 'G')}", f"s{_num(desc, 's')}", f"nbuf{_num(desc, 'nbuf')}",
                "split" if _splits(desc) > 1 else "whole", "slices" if _num(desc, "sl") else "atomics")
    if fam == "cn_wgrad_kernel":  # the dword kernel runs set by set
        return (name, "G1", f"s{_num(desc, 's')}", f"nbuf{_num(desc, 'nbuf')}", "split" if _splits(desc) > 1 else "whole",
                "atomics")
    if fam == "cn_bconv_kernel":
        m = re.search(r" s(\d+)/(\d+)", desc)
        assert m, desc
        return (name, "G>1" if _num(desc, "G") > 1 else "G1", f"cls{_num(desc, 'cls')}", f"taps{_num(desc, 'taps')}",
                f"is{m.group(1)}", f"os{m.group(2)}", f"il{_num(desc, 'il')}", f"st{_num(desc, 'st')}",
                f"fin{_num(desc, 'fin')}")
    if fam == "cn_pretime_kernel":  # the recorded name is <PASS[, reg]>; the description holds all six arguments
        m = re.match(r"pretime(<[^>]*>)", desc)
        assert m, f"cn_pretime_kernel launch without its instantiation: {desc!r}"
        return (fam + m.group(1), name)
    if fam == "cn_bwgrad_kernel":
        return (name, f"s{_num(desc, 's')}", "split" if _num(desc, "split") > 1 else "whole")
    return (name,)


def instantiation(key) -> str:
    return key[0]


def production_facts(key, phase: str) -> T.Tuple[str, ...]:
    """What the model's own calls are ASSUMED to set up around a launch of `key` (phase "step" or "eval"), from reading
    the engine, not from the recording: params.py registers a split-K workspace on every stream it launches on, and a
    training step runs its weight gradients under the deferred slice-sum sink. If the engine stopped doing either, these
    facts would be wrong without any test noticing."""
    fam = instantiation(key).split("<")[0]
    if fam in ("cn_conv_igemm_vec_kernel", "cn_conv_igemm_kernel", "cn_gemm1x1_kernel"):
        return ("ws",)
    if fam in ("cn_wgrad_vec_kernel", "cn_wgrad_vec3_kernel", "cn_wgrad_kernel", "cn_bwgrad_kernel") and phase == "step":
        return ("sink active",)
    return ()


def covers(case_key, production_key) -> bool:
    """Does the exact case that emitted `case_key` run the route `production_key`? Same instantiation, same recorded
    facts (every fact is a self-describing string), and every caller-side fact of the production launch holds for the
    case, which may state more (its workspace size, accumulate)."""
    return instantiation(case_key) == instantiation(production_key) and set(production_key) <= set(case_key)


class Routes:
    """The route keys one test emits, part by part, held against its entry in contraction_routes.CASES.

        routes = Routes("test_conv_exact_gpu.py::test_conv2d_bf16_exact[case3]", tmp_path)
        with routes.part("y", "acc"):      # caller-known facts follow the label
            L.call(...)
        routes.verify()                    # prints the ledger lines, then compares
    """

    def __init__(self, case_id: str, tmp_dir, *facts: str):
        self.case_id, self.tmp_dir = case_id, tmp_dir
        self.facts = tuple(facts)  # caller-known facts of every part of this test
        self.got: T.Dict[str, T.List[T.Tuple[str, ...]]] = {}

    @contextlib.contextmanager
    def part(self, label: str, *facts: str):
        with recording(self.tmp_dir) as launches:
            yield
        keys = self.got.setdefault(label, [])
        for name, desc in launches:
            k = route_key(name, desc) + self.facts + tuple(facts)
            if k not in keys:
                keys.append(k)
        keys.sort()

    def verify(self):
        from contraction_routes import CASES

        print(f"LEDGER {self.case_id!r}: {self.got!r},")
        want = CASES.get(self.case_id)
        assert want is not None, f"route ledger: no CASES entry for {self.case_id}; it emitted {self.got}"
        for label in sorted(set(want) | set(self.got)):
            old, new = sorted(want.get(label, [])), sorted(self.got.get(label, []))
            assert old == new, (f"route changed: {self.case_id} part {label!r}: the ledger has {old}, the launch took {new}"
                                " -- a dispatch rule moved this case; the kernel it used to check may now be unchecked")


def case_id(request) -> str:
    """<test file>::<test name with its parameter id> of the running test."""
    return f"{os.path.basename(str(request.node.fspath))}::{request.node.name}"


# ---------------------------------------------------------------------------------------------------------------------
# the instantiations the built library holds
# ---------------------------------------------------------------------------------------------------------------------

def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cultionet_amd", "csrc",
                        "libcultionet_hip.so")


def compiled_instantiations(families=FAMILIES) -> T.Set[str]:
    """Kernel instantiations of `families` in the symbol table of the built library, spelled as cn_prof_name spells
    them. Raises AssertionError (never skips) when the library or a symbol-table tool is missing."""
    so = library_path()
    assert os.path.exists(so), f"{so} is not built: run make -C cultionet_amd/csrc"
    tool = shutil.which("nm") or shutil.which("llvm-nm") or next(
        (p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None)
    assert tool is not None, "neither nm nor llvm-nm found: the symbol table cannot be read"
    out = subprocess.run([tool, "-C", so], capture_output=True, text=True, check=True).stdout
    pat = re.compile(r"\bvoid ((?:" + "|".join(families) + r")<[^>]*>)\(")
    return {m.group(1) for line in out.splitlines() if "__device_stub__" not in line for m in [pat.search(line)] if m}
