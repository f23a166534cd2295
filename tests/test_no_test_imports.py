"""CPU: nothing imports a test module.  A file pytest collects (test_*.py) holds tests and what only they use; what anything else needs --
another test, the smoke run, oracle/gen_golden_*.py, a script under scratch/ -- lives in a helper module under tests/.  Checked on the
syntax tree of every tracked Python file, so that the scripts that need a GPU or the reference library to run are covered too: no
import of a test_* module, and every name taken from a tests/ helper is one that helper defines."""
import ast
import os
import subprocess

from paths import ROOT

DIRS = ("", "tests", "oracle", "scratch", "profiles", "x264_vs2008_amd")


def tracked_sources():
    """{path relative to the repository: syntax tree} of the *.py files directly in DIRS that git tracks or would track (not ignored); all of
    them where there is no git."""
    try:
        listed = subprocess.run(["git", "ls-files", "--cached", "--others", "--exclude-standard", "*.py"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.split()
    except (OSError, subprocess.CalledProcessError):
        listed = []
    if not listed:
        listed = [os.path.join(d, f) for d in DIRS if os.path.isdir(os.path.join(ROOT, d)) for f in os.listdir(os.path.join(ROOT, d)) if f.endswith(".py")]
    out = {}
    for rel in sorted(listed):
        if os.path.dirname(rel) in DIRS and os.path.exists(os.path.join(ROOT, rel)):
            with open(os.path.join(ROOT, rel)) as f:
                out[rel] = ast.parse(f.read(), rel)
    return out


def is_test_module(name):
    last = name.rsplit(".", 1)[-1]
    return last.startswith("test_") or last.endswith("_test")


def defined_names(tree):
    """Names a module binds at its top level (inside its top-level if / try / with / for blocks too)."""
    names = set()
    todo = list(tree.body)
    while todo:
        node = todo.pop()
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            names |= {(a.asname or a.name).split(".")[0] for a in node.names}
        elif isinstance(node, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
            for t in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                names |= {n.id for n in ast.walk(t) if isinstance(n, ast.Name)}
        else:
            for field in ("body", "orelse", "finalbody", "handlers"):
                todo += getattr(node, field, [])
    return names


def test_nothing_imports_a_test_module_and_helper_names_exist():
    sources = tracked_sources()
    assert "__graft_entry__.py" in sources and "tests/stream_util.py" in sources and any(p.startswith("oracle/gen_golden_") for p in sources), sorted(sources)
    bad = []
    for path, tree in sources.items():
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""] + ["%s.%s" % (node.module, a.name) for a in node.names if node.module == "tests"]
            elif isinstance(node, ast.Call) and getattr(node.func, "attr", getattr(node.func, "id", "")) in ("import_module", "__import__"):
                mods = [a.value for a in node.args[:1] if isinstance(a, ast.Constant) and isinstance(a.value, str)]
            else:
                continue
            bad += ["%s:%d imports %s" % (path, node.lineno, m) for m in mods if is_test_module(m)]
    assert not bad, "test modules are imported:\n  " + "\n  ".join(bad)
    # every name taken from a helper module of tests/ is one it defines
    helpers = {os.path.basename(p)[:-3]: defined_names(t) for p, t in sources.items()
               if os.path.dirname(p) == "tests" and not is_test_module(os.path.basename(p)[:-3]) and os.path.basename(p) != "conftest.py"}
    assert {"paths", "slice_util", "stream_util", "full_batch_util", "mux_cases", "look_cases"} <= set(helpers), sorted(helpers)
    bad, checked = [], 0
    for path, tree in sources.items():
        alias = {}                                      # `import helper as T`: T.name is looked up as well (in every helper the file calls T)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module in helpers and not node.level:
                for a in node.names:
                    checked += 1
                    if a.name != "*" and a.name not in helpers[node.module]:
                        bad.append("%s:%d: tests/%s.py defines no %s" % (path, node.lineno, node.module, a.name))
            elif isinstance(node, ast.Import):
                for a in node.names:
                    if a.name in helpers:
                        alias.setdefault(a.asname or a.name, set()).add(a.name)
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in alias and isinstance(node.ctx, ast.Load):
                checked += 1
                if not any(node.attr in helpers[h] for h in alias[node.value.id]):
                    bad.append("%s:%d: tests/%s.py defines no %s" % (path, node.lineno, " / ".join(sorted(alias[node.value.id])), node.attr))
    assert checked > 100, checked
    assert not bad, "names that their helper module does not define:\n  " + "\n  ".join(bad)
