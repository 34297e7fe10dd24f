"""What dfl_amd/_native.py publishes, hand-written (a parent revision, read with `git show`) against derived from
include/dfl_hip.h (the working tree): every struct class, constant, op kind, EXPORTS, and the argtypes / restype lib() sets.

    python docs/experiments/cabi_from_header/compare.py [parent revision, default 4dcc147] > docs/experiments/cabi_from_header/report.txt

Needs neither a GPU nor the built library (ctypes.CDLL is replaced by a stand-in that records what lib() assigns), and imports
neither torch nor the package's __init__.  Exit status 1 if anything differs beyond the two expected kinds."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
PKG = 'deepfluorolabeling-ipcai2020_amd'
os.environ['DFL_LIB_OVERRIDE'] = os.path.abspath(__file__)        # any file that exists: lib() looks before it loads
os.environ['DFL_TUNE'] = '0'


def load(name, source=None):
    """_native.py as module <name>._native of an empty package over the package directory (source: the parent's text)."""
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(ROOT, PKG)]
    sys.modules[name] = pkg
    if source is None:
        return importlib.import_module(name + '._native')
    mod = types.ModuleType(name + '._native')
    mod.__package__, mod.__file__ = name, os.path.join(ROOT, PKG, '_native.py')
    exec(compile(source, 'parent:_native.py', 'exec'), mod.__dict__)
    return mod


class Fn:
    restype = argtypes = 'unset'

    def __init__(self, call):
        self.call = call

    def __call__(self, *args):
        return self.call(*args)


class Recorder:
    """Stands for the loaded library: every symbol exists, dfl_sizeof answers from the module's own table, and what lib()
    assigns to a function stays readable."""

    def __init__(self, mod):
        order = mod._SIZEOF_ORDER
        self.fns = {'dfl_sizeof': Fn(lambda k: C.sizeof(order[k]) if k < len(order) else -1)}

    def __getattr__(self, name):
        return self.fns.setdefault(name, Fn(lambda *args: 0))


def signatures(mod):
    real, C.CDLL = C.CDLL, lambda path: Recorder(mod)
    try:
        L = mod.lib()
    finally:
        C.CDLL = real
    return {f: (L.fns[f].restype, L.fns[f].argtypes) for f in mod.EXPORTS}


def tname(t):
    if t == 'unset':
        return t
    if issubclass(t, C.Array):
        return '%s[%d]' % (tname(t._type_), t._length_)
    if issubclass(t, C.Structure):
        return 'struct %s (%d bytes)' % (t.__name__, C.sizeof(t))
    return t.__name__


def layout(cls):
    return [(f, getattr(cls, f).offset, getattr(cls, f).size, tname(t)) for f, t in cls._fields_] + [('sizeof', C.sizeof(cls))]


def sig(s):
    res, args = s
    return '%s (%s)' % (tname(res), args if args == 'unset' else ', '.join(tname(a) for a in args))


def public(mod, kind):
    return {k: v for k, v in vars(mod).items() if not k.startswith('_') and kind(v)}


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else '4dcc147'
    text = subprocess.run(['git', 'show', '%s:%s/_native.py' % (rev, PKG)], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    old, new = load('abi_parent', text), load('abi_new')
    unexpected = []

    is_struct = lambda v: isinstance(v, type) and issubclass(v, C.Structure)
    so, sn = public(old, is_struct), public(new, is_struct)
    print('== struct classes: %d in the parent, %d now; fields as (name, offset, size, type)' % (len(so), len(sn)))
    if list(so) != list(sn):
        print('class order differs (parent: order of writing; now: header order)')
    if set(so) != set(sn):
        unexpected.append('classes: only parent %s, only new %s' % (sorted(set(so) - set(sn)), sorted(set(sn) - set(so))))
    n_fields = 0
    for name in sn:
        a, b = layout(so[name]) if name in so else None, layout(sn[name])
        n_fields += len(b) - 1
        print('%s  %s' % (name, 'same' if a == b else 'DIFFERENT'))
        for row in b:
            print('    ' + ' '.join(str(x) for x in row))
        if a != b:
            unexpected.append('layout of %s: parent %s' % (name, a))
    print('%d fields' % n_fields)
    for tab in ('_KIND_OF', '_SIZEOF_ORDER'):
        a, b = getattr(old, tab), getattr(new, tab)
        a, b = ([(k.__name__, v) for k, v in x.items()] if isinstance(x, dict) else [k.__name__ for k in x] for x in (a, b))
        print('%s: %d entries, %s' % (tab, len(b), 'same' if a == b else 'DIFFERENT'))
        if a != b:
            unexpected.append(tab)

    is_int = lambda v: type(v) is int
    co, cn = public(old, is_int), public(new, is_int)
    print('\n== integer constants and op kinds: %d in the parent, %d now' % (len(co), len(cn)))
    for k in cn:
        print('%s = %d%s' % (k, cn[k], '' if k in co else '   (new on the Python side)'))
    for k in co:
        if k not in cn or co[k] != cn[k]:
            unexpected.append('constant %s: parent %d, new %s' % (k, co[k], cn.get(k)))

    print('\n== EXPORTS: %d in the parent, %d now; as sets %s; in order %s' % (
        len(old.EXPORTS), len(new.EXPORTS), 'same' if set(old.EXPORTS) == set(new.EXPORTS) else 'DIFFERENT',
        'same' if old.EXPORTS == new.EXPORTS else 'different (parent: order of writing; now: header order)'))
    if set(old.EXPORTS) != set(new.EXPORTS) or len(old.EXPORTS) != len(new.EXPORTS):
        unexpected.append('EXPORTS')
    print('parent order: ' + ' '.join(old.EXPORTS))
    print('new order:    ' + ' '.join(new.EXPORTS))

    go, gn = signatures(old), signatures(new)
    print('\n== restype (argtypes) set by lib(); "unset" is ctypes\' default: int result, arguments converted by their Python type')
    gained = []
    for f in new.EXPORTS:
        a, b = go[f], gn[f]
        res_same = tname(a[0]) == tname(b[0]) or (a[0] == 'unset' and b[0] is C.c_int)
        if res_same and a[1] != 'unset' and [tname(t) for t in a[1]] == [tname(t) for t in b[1]]:
            print('%s: %s  same' % (f, sig(b)))
        elif res_same and a[1] == 'unset':
            gained.append(f)
            print('%s: %s  (parent: argtypes unset)' % (f, sig(b)))
        else:
            print('%s: %s  DIFFERENT, parent: %s' % (f, sig(b), sig(a)))
            unexpected.append('signature of %s' % f)

    print('\n== result')
    print('functions that gain argtypes: %d: %s' % (len(gained), ' '.join(gained)))
    print('constants new on the Python side: %d: %s' % (len(set(cn) - set(co)), ' '.join(k for k in cn if k not in co)))
    print('other differences: %d' % len(unexpected))
    for u in unexpected:
        print('  ' + u)
    return 1 if unexpected else 0


if __name__ == '__main__':
    sys.exit(main())
