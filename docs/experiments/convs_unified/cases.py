"""Argument blocks of the latency form for the parent-against-new comparisons of this directory (route_sweep.py on the host,
bit_identity.py on the GPU): every case of the case lists of tests/test_gpu_latency_form.py and tests/test_gpu_latency_form_f32.py,
read from the test files themselves, in the three arithmetics (bf16 storage, fp32, bf16x3).

A block is described by a dict and materialised by `build`, which takes an allocator: alloc(name, nbytes, kind) -> address.
The host sweep hands out made-up 256-byte aligned addresses (the queries never read a tensor); the GPU job allocates seeded
device tensors.  Packed weights are random numbers in the packed layout: the comparison needs the same operands, not a model."""
import ast
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
MODES = {'bf16s': 4, 'fp32': 0, 'bf16x3': 1}           # dfl_set_math_mode


def _literal_lists(path):
    """{name: list} of the module-level case lists, the parametrize lists (by test name) and the for-loop tuples (by test name)."""
    tree = ast.parse(open(path).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id.endswith('CASES'):
            out[node.targets[0].id] = ast.literal_eval(node.value)
        if isinstance(node, ast.FunctionDef):
            for d in node.decorator_list:
                if isinstance(d, ast.Call) and getattr(d.func, 'attr', '') == 'parametrize' and not isinstance(d.args[1], ast.Name):
                    out[node.name] = ast.literal_eval(d.args[1])
            for sub in ast.walk(node):
                if isinstance(sub, ast.For) and isinstance(sub.iter, ast.Tuple) and all(isinstance(e, ast.Tuple) for e in sub.iter.elts):
                    out.setdefault(node.name, []).extend(ast.literal_eval(sub.iter))
    return out


def case_lists():
    b = _literal_lists(os.path.join(ROOT, 'tests', 'test_gpu_latency_form.py'))
    f = _literal_lists(os.path.join(ROOT, 'tests', 'test_gpu_latency_form_f32.py'))

    def both(kb, kf):
        seen = []
        for c in list(b[kb]) + list(f[kf]):
            if c not in seen:
                seen.append(c)
        return seen
    return {
        'plain': both('LCASES', 'FCASES'),
        'affine': both('test_latency_form_affine_residual_epilogue', 'test_latency_form_f32_affine_residual_epilogue'),
        'scatter': both('test_latency_form_transposed_scatter', 'test_latency_form_f32_transposed_scatter'),
        'outaff': both('test_output_affine_is_the_consumers_affine_on_load', 'test_output_affine_f32_is_the_consumers_affine_on_load'),
        'pair': both('test_pair_is_the_two_launches', 'test_pair_f32_is_the_two_launches'),
        'first': both('test_first_layer_latency_form_is_the_row_kernel', 'test_first_layer_f32_latency_form_is_the_direct_kernel'),
    }


def specs(mode):
    """The blocks of one arithmetic, as dicts: name, the convolution(s) and the epilogue options."""
    L = case_lists()
    out = []
    for c in L['plain']:
        N, Cin, Cout, H, W, K, s, p = c
        out.append(dict(name='plain %s' % (c,), a=dict(N=N, Cin=Cin, Cout=Cout, H=H, W=W, K=K, stride=s, pad=p, bias=1, relu=1)))
    for c in L['affine']:
        N, Cin, Cout, H, W, K = c
        for acc in (0, 1):
            out.append(dict(name='affine %s acc%d' % (c, acc),
                            a=dict(N=N, Cin=Cin, Cout=Cout, H=H, W=W, K=K, stride=1, pad=K // 2, bias=1, in_aff=1, add=1, add_aff=1, accumulate=acc)))
    for c in L['scatter']:
        N, Ci, Co, H, W = c
        out.append(dict(name='scatter %s' % (c,), a=dict(N=N, Cin=Ci, Cout=4 * Co, H=H, W=W, K=1, stride=1, pad=0, bias=1, scatter=1, ldy=2 * Co)))
    for c in L['outaff']:
        Cin, C_, H, W = c
        out.append(dict(name='outaff producer %s' % (c,), a=dict(N=1, Cin=Cin, Cout=C_, H=H, W=W, K=3, stride=1, pad=1, bias=1, relu=1, out_aff=1)))
        out.append(dict(name='outaff consumer %s' % (c,), a=dict(N=1, Cin=C_, Cout=C_, H=H, W=W, K=3, stride=1, pad=1, bias=1, relu=1, in_aff=1)))
    for c in L['pair']:
        N, Cres, C_, H, W = c
        out.append(dict(name='pair %s' % (c,), a=dict(N=N, Cin=C_, Cout=C_, H=H, W=W, K=3, stride=1, pad=1, bias=1, relu=1),
                        b=dict(N=N, Cin=Cres or 1, Cout=C_, H=H, W=W, K=1, stride=1, pad=0, bias=1, ldy=2 * C_, image=0 if Cres else 1)))
    for c in L['first']:
        N, H, W, C_ = c
        out.append(dict(name='first %s' % (c,), a=dict(N=N, Cin=1, Cout=C_, H=H, W=W, K=3, stride=1, pad=1, bias=1, relu=1, image=1)))
        out.append(dict(name='first outaff %s' % (c,), a=dict(N=N, Cin=1, Cout=C_, H=H, W=W, K=3, stride=1, pad=1, bias=1, relu=1, image=1, out_aff=1)))
    return out


def build(nat, mode, d, alloc, tag):
    """dict -> nat.ConvArgs.  alloc(name, count, kind): kind 'act' (the mode's tensor format), 'f32', 'w' (packed weights: count in BYTES)."""
    bf = mode == 'bf16s'
    image = d.get('image', 0)                        # the 1-channel fp32 image of the network's first block
    a = nat.ConvArgs()
    N, Cin, Ntot, H, W, K = d['N'], d['Cin'], d['Cout'], d['H'], d['W'], d['K']
    s, p = d['stride'], d['pad']
    scat = d.get('scatter', 0)
    Ho, Wo = ((2 * H, 2 * W) if scat else ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1))
    Cout = Ntot // 4 if scat else Ntot
    ldy = d.get('ldy', Cout)
    a.N, a.Hin, a.Win, a.Cin, a.ldx = N, H, W, Cin, Cin
    a.KH, a.KW, a.stride, a.pad = K, K, s, p
    a.Hout, a.Wout, a.Ntot, a.ldy = Ho, Wo, Ntot, ldy
    a.relu, a.accumulate, a.scatter2x2 = d.get('relu', 0), d.get('accumulate', 0), scat
    a.latency_form = 1
    a.x_bf16, a.y_bf16 = (0 if image else int(bf)), int(bf)
    a.w_split = 0 if image else (2 if bf else (1 if mode == 'bf16x3' else 0))
    Kt = K * K * Cin
    wbytes = ((Kt + 15) // 16 * Ntot * 16 * 2) if (bf and not image) else ((Kt + 3) // 4 * Ntot * 16)
    a.x = alloc(tag + '.x', N * H * W * Cin, 'f32' if image else 'act')
    a.w = alloc(tag + '.w', wbytes, 'w_bf16' if a.w_split else 'w_f32')
    a.y = alloc(tag + '.y', N * Ho * Wo * ldy, 'out')
    if d.get('bias'):
        a.bias = alloc(tag + '.bias', Cout, 'f32')
    if d.get('in_aff'):
        a.in_scale, a.in_shift = alloc(tag + '.isc', Cin, 'scale'), alloc(tag + '.ish', Cin, 'f32')
    if d.get('add'):
        a.add, a.ldadd = alloc(tag + '.add', N * Ho * Wo * Ntot, 'act'), Ntot
    if d.get('add_aff'):
        a.add_scale, a.add_shift = alloc(tag + '.asc', Ntot, 'scale'), alloc(tag + '.ash', Ntot, 'f32')
    if d.get('out_aff'):
        a.out_scale, a.out_shift = alloc(tag + '.osc', Cout, 'scale'), alloc(tag + '.osh', Cout, 'f32')
    return a


def pair_link(a, b, alloc, tag):
    """b = the block's 1x1 convolution with '+ BN(y1)' of a's output."""
    b.add, b.ldadd = a.y, a.ldy
    b.add_scale, b.add_shift = alloc(tag + '.pasc', b.Ntot, 'scale'), alloc(tag + '.pash', b.Ntot, 'f32')


def copy_args(nat, st):
    return nat.ConvArgs.from_buffer_copy(bytes(st))


def paper_blocks(nat, dfl_amd, torch, size, device):
    """The convolution blocks of the eval-mode paper plan at size x size, batch 1, in the current arithmetic: ([ConvArgs], [(a, b)], plan)."""
    import bench
    from dfl_amd.plan import UNetPlan
    torch.manual_seed(5)
    net = dfl_amd.UNet(**bench.PAPER).eval()
    P, B = net._state()
    plan = UNetPlan(net._cfg, P, B, 1, size, size, False, False, device)
    convs, pairs = [], []
    for st in plan.fwd.structs:
        if isinstance(st, nat.ConvArgs):
            convs.append(st)
        elif isinstance(st, nat.ConvPairArgs):
            a, b = nat.ConvArgs.from_address(st.a), nat.ConvArgs.from_address(st.b)
            pairs.append((a, b))
            convs += [a, b]
    return convs, pairs, (net, plan)
