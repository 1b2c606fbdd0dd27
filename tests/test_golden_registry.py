"""Every committed reference fixture has a generator: tests/golden/make_golden.py::RECIPES names each tests/golden/*.npz, so
`make_golden.py --check NAME` can regenerate it and compare bit for bit.  The file is parsed, not imported (importing it imports the reference)."""
import ast
import glob
import os

from conftest import GOLDEN


def _recipes():
    tree = ast.parse(open(os.path.join(GOLDEN, 'make_golden.py')).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == 'RECIPES' for t in node.targets):
            assert isinstance(node.value, ast.Dict), 'RECIPES is expected to be a dict literal'
            keys = [ast.literal_eval(k) for k in node.value.keys]
            assert len(keys) == len(set(keys)), 'a fixture name appears twice in RECIPES'
            return set(keys)
    raise AssertionError('make_golden.py defines no RECIPES')


def test_every_fixture_has_a_recipe():
    fixtures = {os.path.basename(p)[:-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, '*.npz'))}
    assert fixtures
    missing = sorted(fixtures - _recipes())
    assert not missing, 'fixtures without a RECIPES entry in make_golden.py: %s' % ', '.join(missing)
