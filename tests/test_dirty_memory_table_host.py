"""Completeness of tests/test_gpu_dirty_memory.py, without a device: every public function or method of mvsdf_amd/*.py that allocates uninitialised
memory -- torch.empty( or torch.empty_like( in its own body or in a private helper of the same module that it reaches -- is a key of that file's
CASES table, or is in NOT_COVERED with its reason.  A new entry point therefore fails here until it runs on dirty memory."""
import ast
import glob
import inspect
import importlib
import os
import re
import textwrap

from conftest import ROOT

import test_gpu_dirty_memory as D

ALLOC = re.compile(r'\btorch\.empty(_like)?\(')
OTHER_SPELLINGS = re.compile(r'\.new_empty\(|\bempty_strided\(|\btorch\.(Float|Double|Int|Long|Byte|Half|BFloat16)Tensor\(\s*[\d)]|\.resize_\(')
NOT_COVERED_SHARE = 0.10                                                     # raised only as the module docstring of test_gpu_dirty_memory.py records


def _modules():
    return sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, 'mvsdf_amd', '*.py')) if not os.path.basename(p).startswith('_'))


def _callables(mod):
    """{'name' or 'Class.name': function} defined in `mod` itself"""
    out = {}
    for name, obj in vars(mod).items():
        if inspect.isfunction(obj) and obj.__module__ == mod.__name__:
            out[name] = obj
        elif inspect.isclass(obj) and obj.__module__ == mod.__name__:
            for mname, m in vars(obj).items():
                f = m.__func__ if isinstance(m, (staticmethod, classmethod)) else m.fget if isinstance(m, property) else m
                if inspect.isfunction(f):
                    out['%s.%s' % (name, mname)] = f
    return out


def _source(fn):
    try:
        return textwrap.dedent(inspect.getsource(fn))
    except (OSError, TypeError):                                             # generated code (a dataclass's __init__): nothing of ours to read
        return ''


def _called_names(fn):
    """every bare name and every attribute name the body of `fn` mentions: a superset of the helpers it calls"""
    tree = ast.parse(_source(fn))
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Name):
            names.add(node.id)
        elif isinstance(node, ast.Attribute):
            names.add(node.attr)
    return names


def _public(key):
    parts = key.split('.')
    if len(parts) == 1:
        return not key.startswith('_')
    return not parts[0].startswith('_') and (not parts[1].startswith('_') or parts[1] in ('__init__', '__call__'))


def allocating_entries():
    """{'module.entry': the names through which it reaches an allocation} over mvsdf_amd/*.py"""
    found = {}
    for modname in _modules():
        mod = importlib.import_module('mvsdf_amd.' + modname)
        fns = _callables(mod)
        by_last = {}
        for key, f in fns.items():
            by_last.setdefault(key.split('.')[-1], []).append(key)
            if '.' in key:
                by_last.setdefault(key.split('.')[0], [])
        for cls in {k.split('.')[0] for k in fns if '.' in k}:               # Class(...) reaches Class.__init__
            if cls + '.__init__' in fns:
                by_last.setdefault(cls, []).append(cls + '.__init__')
        direct = {k for k, f in fns.items() if ALLOC.search(_source(f))}
        calls = {k: _called_names(f) for k, f in fns.items()}
        for key in fns:
            if not _public(key):
                continue
            seen, todo, via = {key}, [key], []
            while todo:
                k = todo.pop()
                if k in direct:
                    via.append(k)
                for name in calls[k]:
                    for k2 in by_last.get(name, ()):
                        private = k2.split('.')[-1].startswith('_') or k2.split('.')[0].startswith('_')
                        if k2 not in seen and private:                       # only through private helpers: a public callee is an entry of its own
                            seen.add(k2)
                            todo.append(k2)
            if via:
                found['%s.%s' % (modname, key)] = sorted(via)
    return found


def test_every_allocating_entry_point_is_in_the_table_or_exempt_with_a_reason():
    found = allocating_entries()
    assert len(found) >= 60, len(found)                                      # the walk itself works
    for probe in ('cloud.knn_mean_distance', 'bundle.normal_blocks', 'registration.NearestTree.__init__', 'raster.rasterize', 'ops.trace'):
        assert probe in found, probe
    missing = sorted(k for k in found if k not in D.CASES and k not in D.NOT_COVERED)
    assert not missing, missing
    stale = sorted(k for k in list(D.CASES) + list(D.NOT_COVERED) if k not in found)
    assert not stale, stale                                                  # a renamed entry point does not leave a dead row behind
    assert not set(D.CASES) & set(D.NOT_COVERED)


def test_exemptions_are_few_and_give_a_reason():
    found = allocating_entries()
    assert len(D.NOT_COVERED) <= NOT_COVERED_SHARE * len(found), (len(D.NOT_COVERED), len(found))
    for key, reason in D.NOT_COVERED.items():
        assert key.split('.')[0] not in D.MODULES, key                       # none from the workspace-carving modules
        assert reason.startswith('allocates on the host only') or reason.startswith('covered by test_gpu_diff_fp64'), (key, reason)


def test_every_case_is_a_function_of_the_file_and_runs_under_all_three_patterns():
    assert set(D.POISON_PATTERNS) == {0xff, 0x00, 0x5a}
    for key, names in D.CASES.items():
        assert names, key
        for name in names:
            assert callable(getattr(D, name)) and key in D.CASE_KEYS[name], (key, name)
    marks = [m for m in D.test_on_dirty_memory.pytestmark if m.name == 'parametrize']
    assert sorted(marks[0].args[1]) == sorted((name, p) for name in D.CASE_KEYS for p in D.POISON_PATTERNS)


def test_the_library_has_no_other_uninitialised_allocation_spelling():
    """helpers.dirty_allocations patches torch.empty and torch.empty_like; the library must not allocate uninitialised memory any other way"""
    for path in glob.glob(os.path.join(ROOT, 'mvsdf_amd', '**', '*.py'), recursive=True):
        with open(path) as f:
            src = f.read()
        assert not OTHER_SPELLINGS.search(src), (path, OTHER_SPELLINGS.search(src).group(0))
        assert not re.search(r'from torch import .*\bempty', src), path       # a bound name would escape the patch
