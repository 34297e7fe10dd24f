"""Reader of include/dfl_hip.h: the header is the only statement of the C ABI, and the ctypes binding (_native.py) is computed
from it at import -- constants, struct layouts and function signatures.

The reader knows exactly the C the header uses and refuses everything else (HeaderError names the line): a construct it
passed over in silence would be a part of the contract the binding does not follow.
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'include', 'dfl_hip.h')
RENAME = {'in': 'inp'}     # field names that are Python keywords

_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64,
            'float': C.c_float, 'double': C.c_double}
_POINTEES = ('void', 'char', 'unsigned char', 'uint8_t')     # types the header names only behind a pointer
# one declarator up to its separator: [type words] [* [const]]... name [dimensions]
_DECL = re.compile(r'\s*([\w\s]*)((?:\*\s*(?:const\b\s*)?)*)(?<!\w)(\w+)\s*((?:\[[^\]]*\]\s*)*)([;,]|$)')
_EXPR = set('abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_0123456789 \t\n()+-*/%<>|&^~')


class HeaderError(ValueError):
    pass


def camel(name):
    """dfl_conv_args -> ConvArgs"""
    return ''.join(w.capitalize() for w in name[4:].split('_'))


def parse(text, name='dfl_hip.h'):
    """(constants, structs, functions) of a header text: {DFL_NAME: int}, {dfl_name: ctypes.Structure subclass} and
    {dfl_name: (restype, argtypes)}, each in declaration order."""
    consts, structs, funcs = {}, {}, {}
    types = dict(_SCALARS, **dict.fromkeys(_POINTEES))     # C type name -> ctypes type (None: pointee only)
    # comments go, their line breaks stay; below, preprocessor lines are blanked in place: positions keep their lines
    text = re.sub(r'/\*.*?\*/', lambda m: ' ' + '\n' * m.group().count('\n'), text, flags=re.S)

    def fail(pos, what):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        line = text.count('\n', 0, pos) + 1
        raise HeaderError('%s:%d: %s: %s' % (name, line, what, text.split('\n')[line - 1].strip()))

    def integer(expr, pos):
        try:                                   # names, numbers and integer operators only: nothing that could call or index
            v = eval(expr.strip().replace('/', '//'), {'__builtins__': {}}, consts) if set(expr) <= _EXPR else None
        except Exception:
            v = None
        if type(v) is not int:
            fail(pos, 'not an integer expression')
        return v

    def ctype(words, stars, pos):
        if words not in types:                 # as written (`const float `): looked up without const once, then remembered
            types[words] = types.get(' '.join(w for w in words.split() if w != 'const'), KeyError)
        t = types[words]
        if t is KeyError:
            fail(pos, 'unknown type %r' % words.strip())
        if stars:
            return C.c_void_p
        if t is None:
            fail(pos, '%s by value' % words.strip())
        return t

    def declarators(s, base, carry):
        """(name, ctypes type) of the fields of a struct body (carry = ',': `int32_t a, b;`) or the parameters of a prototype."""
        pos, words, end = 0, '', len(s.rstrip())
        while pos < end:
            m = _DECL.match(s, pos)
            typ, stars, field, dims, sep = m.groups() if m else ('', '', '', '', '')
            if not m or not (typ.strip() or words):
                rest = s[pos:].split(';')[0]
                fail(base + pos, 'bit-field' if ':' in rest else 'cannot read declarator %r' % rest.split(',')[0].strip())
            words = typ if typ.strip() else words
            t = ctype(words, stars, base + m.start(3))
            if dims and carry is None:
                fail(base + m.start(4), 'array parameter')
            for dim in reversed(dims.replace(']', ' ').split('[')[1:]):
                t = t * integer(dim, base + m.start(4))
            yield RENAME.get(field, field), t
            words = words if sep == carry else ''
            pos = m.end()

    # preprocessor lines: the include guard, #include and the extern "C" block are passed over, #define DFL_* is a constant
    guard = re.search(r'^#ifndef (\w+)\n#define \1$', text, re.M)
    allowed = ('#ifndef %s' % guard.group(1), '#define %s' % guard.group(1), '#endif') if guard else ()
    text = re.sub(r'^#ifdef __cplusplus\n[^#]*#endif$', lambda m: '\n'.join(' ' * len(ln) for ln in m.group().split('\n')),
                  text, flags=re.M)

    def directive(m):
        s, define = m.group().strip(), re.fullmatch(r'\s*#\s*define\s+(DFL_\w+)\s+(\S.*)', m.group())
        if define:
            consts[define.group(1)] = integer(define.group(2), m.start())
        elif not (s in allowed or (s.startswith('#include <') and s.endswith('.h>'))):
            fail(m.start(), 'unsupported preprocessor line')
        return ' ' * len(m.group())
    code = re.sub(r'^[ \t]*#.*$', directive, text, flags=re.M)

    # declarations: everything between two ';' outside braces
    depth, start = 0, 0
    for m in re.finditer(r'[{};]', code + ';'):
        depth += {'{': 1, '}': -1, ';': 0}[m.group()]
        if m.group() != ';' or depth:
            continue
        at = start + len(code[start:m.start()]) - len(code[start:m.start()].lstrip())
        stmt, start = code[at:m.start()].rstrip(), m.end()
        if not stmt:
            continue
        typedef = stmt.startswith('typedef')
        op = typedef and re.fullmatch(r'typedef\s+(?:void|struct\s+\w+)\s*\*\s*(\w+)', stmt)
        en = typedef and re.fullmatch(r'typedef\s+enum\s*\{([^{}]*)\}\s*(\w+)', stmt)
        st = typedef and re.fullmatch(r'typedef\s+struct\s*\{(.*)\}\s*(dfl_\w+)', stmt, re.S)
        fn = not typedef and re.fullmatch(r'([^(){}]*?)(dfl_\w+)\s*\(([^(){}]*)\)', stmt)
        if op:
            types[op.group(1)] = C.c_void_p
        elif en:
            v, pos = -1, at + en.start(1)
            for e in en.group(1).split(','):
                one = re.fullmatch(r'\s*(DFL_\w+)\s*(?:=(.*))?', e, re.S) or fail(pos, 'cannot read enumerator')
                v = consts[one.group(1)] = integer(one.group(2), pos) if one.group(2) else v + 1
                pos += len(e) + 1
            types[en.group(2)] = C.c_int
        elif st:
            if '{' in st.group(1):
                fail(at + st.start(1) + st.group(1).index('{'), 'nested struct or union')
            cls = type(camel(st.group(2)), (C.Structure,), {'_fields_': list(declarators(st.group(1), at + st.start(1), ','))})
            types[st.group(2)] = structs[st.group(2)] = cls
        elif fn:
            r = _DECL.fullmatch(fn.group(1) + 'f')       # the return type read as the type of a declarator `f`
            if not r or r.group(4):
                fail(at, 'cannot read return type')
            res = C.c_char_p if r.group(2) and r.group(1).split() == ['const', 'char'] else ctype(r.group(1), r.group(2), at)
            params = '' if fn.group(3).strip() == 'void' else fn.group(3)
            args = [t for _, t in declarators(params, at + fn.start(3), None)]
            funcs[fn.group(2)] = (res, args)
        else:
            fail(at, 'unsupported declaration')
    return consts, structs, funcs


def load(path=HEADER):
    with open(path) as f:
        return parse(f.read(), os.path.basename(path))
