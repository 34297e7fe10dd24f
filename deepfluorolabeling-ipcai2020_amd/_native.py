"""ctypes binding of libdfl_hip.so (C ABI declared in include/dfl_hip.h).

Nothing of the ABI is restated here: the struct classes, the constants, the op kinds, EXPORTS and every function's argtypes /
restype are computed from the header when this module is imported (_cabi.py).  A header struct dfl_<name> is the class
CamelCase(<name>) (dfl_conv_args -> ConvArgs), a constant or enumerator DFL_<NAME> is <NAME> (DFL_OP_CONV -> OP_CONV); the one
field whose name Python reserves is renamed (dfl_resample_args.in -> inp).  Hand-written is only what the header does not say:
which struct belongs to which op kind, the order of the library's dfl_sizeof table, and the calling helpers.

The library is the product: there is no CPU or PyTorch fallback.  If it is missing, loading fails loudly.
"""
import ctypes as C
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DFL_LIB_OVERRIDE') or os.path.join(_HERE, 'lib', 'libdfl_hip.so')   # override: docs/experiments variant builds

i32, i64, f32 = C.c_int32, C.c_int64, C.c_float
fp = C.c_void_p   # every device pointer is passed as a plain address

_CONSTANTS, _STRUCTS, _FUNCTIONS = _cabi.load()
globals().update({name[len('DFL_'):]: value for name, value in _CONSTANTS.items()})     # PACK_PLAIN, AUG_*, OP_*, BN_R, ...
globals().update({cls.__name__: cls for cls in _STRUCTS.values()})                      # ConvArgs, PackJob, Op, ...
EXPORTS = list(_FUNCTIONS)

CONV_CFG_LATENCY = 39      # dfl_conv_config: 16 + this = the latency form (csrc/convp.h: CONVS_TILE)

_KIND_OF = {ConvArgs: OP_CONV, WgradArgs: OP_WGRAD, SumPartialsArgs: OP_SUM_PARTIALS, PackArgs: OP_PACK,
            BnFinalizeArgs: OP_BN_FINALIZE, BnEvalArgs: OP_BN_EVAL, ColstatsArgs: OP_COLSTATS,
            BnBwdFinalizeArgs: OP_BN_BWD_FINALIZE, BnReluBwdArgs: OP_BN_RELU_BWD,
            ReducePartialsArgs: OP_REDUCE_PARTIALS, AffineCopyArgs: OP_AFFINE_COPY, HeadFwdArgs: OP_HEAD_FWD,
            HeadBwdArgs: OP_HEAD_BWD, MemsetArgs: OP_MEMSET, ReduceBatchArgs: OP_REDUCE_BATCH, BnLiveArgs: OP_BN_FINALIZE_LIVE, BnBwdLiveArgs: OP_BN_BWD_FINALIZE_LIVE,
            ConvPairArgs: OP_CONV_PAIR}

# the table of dfl_sizeof (csrc/api.hip), which the header does not state as code: lib() holds every size against it
_SIZEOF_ORDER = [ConvArgs, WgradArgs, PackJob, BnFinalizeArgs, ColstatsArgs, BnBwdFinalizeArgs, BnReluBwdArgs,
                 AffineCopyArgs, PoolArgs, HeadFwdArgs, HeadBwdArgs, LossArgs, EnsembleArgs, Op, ReduceJob, PrepArgs, EstLandsArgs,
                 UpsampleArgs, AugmentArgs, AugmentItem, OverlayArgs, ResamplePlan, ResampleArgs, FullresArgs, MeshMcArgs, MeshDecodeArgs,
                 MeshTopoArgs, MeshCsrArgs, MeshSmoothArgs, MeshXformArgs, MeshNormalsArgs, MeshQuadricsArgs,
                 MeshCollapseKeysArgs, MeshCollapseSelectArgs, MeshCollapseApplyArgs, PreprocProjsArgs, PreprocSegsArgs,
                 RestoreLabelsArgs, SimPrepareArgs, SimGradnccArgs, ExposeArgs, ToolsCapsule, ToolsArgs, SimMiPrepareArgs, SimMiArgs, SimMiBwdArgs,
                 SimPatchPrepareArgs, SimPatchGradnccArgs, RasterMesh, RasterArgs,
                 SimGradnccBwdArgs, SimPatchWeightsArgs, SimPatchEvalArgs, DrrPoseGradArgs, SimBankGradnccArgs, SimBankGradnccBwdArgs, SimPatchBankGradnccArgs, DrrObject, DrrArgs,
                 OptimPackArgs]


class DflError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DflError('libdfl_hip.so not found at %s -- build it with __graft_entry__.build() '
                       '(csrc/build.sh); there is no fallback path' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise DflError('libdfl_hip.so does not export %s' % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _FUNCTIONS[name]      # the header's prototype
    for k, cls in enumerate(_SIZEOF_ORDER):
        if L.dfl_sizeof(k) != C.sizeof(cls):
            raise DflError('struct mirror %s has size %d, library says %d' % (cls.__name__, C.sizeof(cls), L.dfl_sizeof(k)))
    _lib = L
    if os.environ.get('DFL_TUNE', '1') != '0':
        load_tuning(L, TUNE_PATH)
    return L


TUNE_PATH = os.environ.get('DFL_TUNE_FILE') or os.path.join(_HERE, 'tune', 'gfx950_convp.txt')


def load_tuning(L, path):
    """Geometry table of the bf16 convolution, measured on the device by tools/tune_convp.py: one layer per line,
    10 key integers (N Hin Win Cin Ntot KH KW stride pad scatter) and 5 geometry integers (include/dfl_hip.h:
    dfl_conv_tune_add).  Layers that are not listed keep the cost model's choice.  Returns the number of entries."""
    if not os.path.exists(path):
        return 0
    n = 0
    with open(path) as f:
        for line in f:
            line = line.split('#')[0].split()
            if len(line) != 15:
                continue
            v = (i32 * 15)(*[int(t) for t in line])
            if L.dfl_conv_tune_add(C.addressof(v), C.addressof(v) + 40) < 0:
                raise DflError('bad tuning entry in %s: %s' % (path, ' '.join(line)))
            n += 1
    return n


def check(rc, what=''):
    if rc < 0:
        raise DflError('%s failed (%d): %s' % (what or 'libdfl_hip call', rc, lib().dfl_last_error().decode()))
    return rc


def ptr(t):
    """Device address of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def byref(s):
    return C.addressof(s)


def call(fn_name, args_struct, stream):
    return check(getattr(lib(), fn_name)(C.addressof(args_struct), stream), fn_name)


class Graph:
    """An instantiated hipGraph of (part of) a Program; keeps the program (argument structs, tensors) alive."""

    def __init__(self, handle, program):
        self.handle, self.program = handle, program

    def launch(self, stream):
        check(lib().dfl_graph_launch(self.handle, stream), 'dfl_graph_launch')

    @property
    def nodes(self):
        return lib().dfl_graph_nodes(self.handle)

    def __del__(self):
        try:
            if self.handle and _lib is not None:
                _lib.dfl_graph_destroy(self.handle)
        except Exception:
            pass
        self.handle = None


class Program:
    """A recorded list of library calls replayed by dfl_exec (one ctypes transition per replay)."""

    def __init__(self):
        self.structs = []      # keeps the argument structs alive
        self.kinds = []
        self.streams = []      # 0 = the caller's stream, 1.. = library side streams (dfl_op.stream)
        self.volatile = []     # ops whose argument block is rewritten between replays (caller-owned addresses): never captured
        self._ops = None
        self.keep = []         # tensors referenced by raw pointers
        self._chunks = {}      # (start, count) -> [(first op, count, Graph or None)], see run_graphed

    def add(self, args_struct, kind=None, stream=0, volatile=False):
        self.structs.append(args_struct)
        self.kinds.append(kind if kind is not None else _KIND_OF[type(args_struct)])
        self.streams.append(stream)
        self.volatile.append(bool(volatile))
        self._ops = None
        self._chunks = {}
        return args_struct

    def insert(self, index, args_struct, kind=None, stream=0, volatile=False):
        """Like add(), in front of op `index`."""
        self.structs.insert(index, args_struct)
        self.kinds.insert(index, kind if kind is not None else _KIND_OF[type(args_struct)])
        self.streams.insert(index, stream)
        self.volatile.insert(index, bool(volatile))
        self._ops = None
        self._chunks = {}
        return args_struct

    def pop(self):
        """Take the last op back (its argument struct is returned)."""
        self.kinds.pop()
        self.streams.pop()
        self.volatile.pop()
        self._ops = None
        self._chunks = {}
        return self.structs.pop()

    def record(self, event, stream=0):
        """Record library event `event` on `stream` (DFL_OP_RECORD)."""
        return self.add(SyncArgs(event=event), OP_RECORD, stream)

    def wait(self, event, stream=0):
        """Make `stream` wait for library event `event` (DFL_OP_WAIT)."""
        return self.add(SyncArgs(event=event), OP_WAIT, stream)

    def add_pool(self, args_struct, backward):
        return self.add(args_struct, OP_POOL_BWD if backward else OP_POOL_FWD)

    def extend(self, other):
        for s, k, st, v in zip(other.structs, other.kinds, other.streams, other.volatile):
            self.add(s, k, st, v)
        self.keep.extend(other.keep)

    def __len__(self):
        return len(self.structs)

    def _build(self):
        arr = (Op * len(self.structs))()
        for i, (s, k) in enumerate(zip(self.structs, self.kinds)):
            arr[i].kind = k
            arr[i].stream = self.streams[i]
            arr[i].args = C.addressof(s)
        self._ops = arr

    def run_timed(self, stream):
        """Replay with a hipEvent pair around every op (on `stream`); returns the per-op milliseconds."""
        if self._ops is None:
            self._build()
        n = len(self.structs)
        ms = (C.c_float * n)()
        check(lib().dfl_exec_timed(C.addressof(self._ops), n, stream, C.addressof(ms)), 'dfl_exec_timed')
        return list(ms)

    def capture(self, stream, start=0, count=None):
        """hipGraph of ops [start, start + count) (dfl_graph_capture): nothing runs now; Graph.launch(stream) replays."""
        if self._ops is None:
            self._build()
        n = len(self.structs) - start if count is None else count
        h = C.c_void_p()
        check(lib().dfl_graph_capture(C.addressof(self._ops) + start * C.sizeof(Op), n, stream, C.addressof(h)),
              'dfl_graph_capture')
        return Graph(h.value, self)

    MIN_GRAPH_OPS = 2

    def graph_chunks(self, stream, start=0, count=None):
        """Cut ops [start, start + count) into maximal runs that one hipGraph can stand for -- ops whose argument blocks do
        not change between replays -- and the volatile ops in between, which stay plain launches in program order.  Side-stream
        ops and event record / wait do not cut: the executor joins every range at its end (include/dfl_hip.h, "Side
        streams"), so a run is one forked graph.  Graphs are captured here, once per range."""
        n = len(self.structs) - start if count is None else count
        key = (start, n)
        chunks = self._chunks.get(key)
        if chunks is None:
            chunks, i, end = [], start, start + n
            while i < end:
                plain = self.volatile[i]
                j = i + 1
                while j < end and self.volatile[j] == plain:
                    j += 1
                if not plain and sum(1 for k in self.kinds[i:j] if k not in (OP_RECORD, OP_WAIT)) >= self.MIN_GRAPH_OPS:
                    chunks.append((i, j - i, self.capture(stream, i, j - i)))
                else:
                    chunks.append((i, j - i, None))
                i = j
            self._chunks[key] = chunks
        return chunks

    def run_graphed(self, stream, start=0, count=None):
        """Replay ops [start, start + count): hipGraph launches for the capturable runs, dfl_exec for the rest."""
        if not self.structs:
            return
        for first, cnt, graph in self.graph_chunks(stream, start, count):
            if graph is not None:
                graph.launch(stream)
            else:
                self.run(stream, first, cnt)

    def run(self, stream, start=0, count=None):
        if not self.structs:
            return
        if self._ops is None:
            self._build()
        n = len(self.structs) - start if count is None else count
        base = C.addressof(self._ops) + start * C.sizeof(Op)
        check(lib().dfl_exec(base, n, stream), 'dfl_exec')
