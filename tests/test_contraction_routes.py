"""Host-side consistency of the route ledger (tests/contraction_routes.py); needs the built library, no GPU.

COMPILED must be what the library's symbol table holds, every compiled instantiation must be the route of an exact
case or carry a quoted reason why no call can select it, every production route must be taken by an exact case, and
every ledger id must name a test that exists, with all its parameter sets. What this file cannot see: a part line
(say one 'dx' row) deleted from an entry whose keys other cases also emit fails here only if it was the last to reach
an instantiation or a production route; the case itself fails on the GPU (Routes.verify compares part by part).
"""
import os
import re
import subprocess
import sys

import contraction_routes as CR
import route_ledger as RL

TESTS = os.path.dirname(os.path.abspath(__file__))


def _case_keys():
    return [k for parts in CR.CASES.values() for keys in parts.values() for k in keys]


def test_compiled_is_the_symbol_table():
    built = RL.compiled_instantiations(CR.FAMILIES)
    listed = set(CR.COMPILED)
    assert len(listed) == len(CR.COMPILED), "COMPILED lists an instantiation twice"
    assert built == listed, (f"in the library but not in COMPILED: {sorted(built - listed)}; "
                             f"in COMPILED but not in the library: {sorted(listed - built)}")


def test_every_instantiation_is_reached_or_accounted_for():
    reached = {RL.instantiation(k) for k in _case_keys()}
    by_inst = {}
    for cid, parts in CR.CASES.items():
        for keys in parts.values():
            for k in keys:
                if cid not in by_inst.setdefault(RL.instantiation(k), []):
                    by_inst[RL.instantiation(k)].append(cid)
    for inst in CR.COMPILED:  # (-s: the ledger table, instantiation -> exact cases)
        print(f"TABLE {inst}: " + (f"{len(by_inst[inst])} exact cases, first {by_inst[inst][0]}" if inst in by_inst else
                                   "unreachable" if inst in CR.UNREACHABLE else "NOT REACHED"))
    for inst in CR.COMPILED:
        where = [name for name, held in (("CASES", inst in reached), ("UNREACHABLE", inst in CR.UNREACHABLE)) if held]
        assert len(where) == 1, f"{inst}: expected in exactly one of CASES and UNREACHABLE; found in {where}"
    for inst in CR.UNREACHABLE:
        assert inst in CR.COMPILED, f"{inst} is called unreachable but not compiled"
    for inst in reached:
        fam = inst.split("<")[0]
        assert fam not in CR.FAMILIES or inst in CR.COMPILED, f"an exact case records {inst}, which is not compiled"


def test_unreachable_quotes_its_condition():
    for inst, why in CR.UNREACHABLE.items():
        m = re.match(r"(\S+\.hip), (\w+): `(.+)`", why)
        assert m, f"{inst}: the reason must read '<file>, <function>: `<condition>` ...', got {why!r}"
        path = os.path.join(os.path.dirname(TESTS), "cultionet_amd", "csrc", m.group(1))
        assert os.path.exists(path), path
        src = open(path).read()
        assert m.group(2) in src and m.group(3) in src, f"{inst}: {m.group(1)} no longer holds `{m.group(3)}`"


def test_production_routes_are_taken_by_exact_cases():
    keys = _case_keys()
    assert CR.PRODUCTION, "no production configuration recorded"
    for config, phases in CR.PRODUCTION.items():
        for phase, prod in phases.items():
            for k in prod:
                assert RL.instantiation(k) not in CR.UNREACHABLE, (config, phase, k)
                assert any(RL.covers(c, k) for c in keys), f"{config} {phase}: no exact case takes the route {k}"


def _collected(modules):
    """{module: test ids (name[param id])} that pytest collects from tests/<module>, in ONE child process, without
    running anything."""
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] +
                       [os.path.join(TESTS, m) for m in modules], capture_output=True, text=True, cwd=os.path.dirname(TESTS))
    assert r.returncode == 0, f"collecting {modules} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    out = {m: set() for m in modules}
    for line in r.stdout.splitlines():
        path, sep, name = line.partition("::")
        if sep and os.path.basename(path) in out:
            out[os.path.basename(path)].add(name)
    return out


def test_every_case_id_names_a_test():
    by_module = {}
    for cid in CR.CASES:
        module, _, name = cid.partition("::")
        by_module.setdefault(module, []).append(name)
    assert by_module, "the ledger holds no case"
    collected = _collected(sorted(by_module))
    for module, names in sorted(by_module.items()):
        have = collected[module]
        missing = [n for n in names if n not in have]
        assert not missing, f"{module}: the ledger names tests that do not exist: {missing}"
        # a test function the ledger knows is known with every one of its parameter sets
        functions = {n.split("[")[0] for n in names}
        absent = sorted(n for n in have if n.split("[")[0] in functions and n not in names)
        assert not absent, f"{module}: cases without a ledger entry: {absent}"
