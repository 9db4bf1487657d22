"""Shared by tests/test_bf16x1_act.py and tests/test_bf16x1_act_gpu.py: a trunk handle without weights, the block walk of csrc/backbone.hip's
forward_lane restated from frtm_backbone_conv_info, and the format rule of the bf16x1_act mode (csrc/trunk_route.h: act_plan) restated tensor by
tensor from frtm_backbone_conv_route's answers.  Imports no test module."""
import ctypes
import os

BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}
BF16_LAYOUTS = (6, 7, 8)                    # FRTM_WLAYOUT_BF16X1, _BF16X1_3X3, _BF16X1_3X3_S2
MODES = {'fp32': (0, 0, 0), 'bf16x3': (3, 0, 0), 'bf16x1': (1, 0, 0), 'bf16x1_3x3': (1, 1, 0), 'bf16x1_act': (1, 1, 1)}     # pieces, 3x3 flag, storage flag


def lib():
    from frtm_vos_amd import _hip
    return _hip.lib()


class Trunk:
    """A trunk handle that holds no weights; env: variables set around frtm_backbone_create (the only moment the library reads them)."""

    def __init__(self, arch, env=None, bb=None):
        self.arch, self.bb, self.own = arch, bb if bb is not None else ctypes.c_void_p(), bb is None
        if not self.own:
            return
        old = {k: os.environ.get(k) for k in env or {}}
        os.environ.update(env or {})
        try:
            assert lib().frtm_backbone_create(arch, ctypes.byref(self.bb)) == 0
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.own:
            lib().frtm_backbone_destroy(self.bb)

    def mode(self, name):
        pieces, flag, act = MODES[name]
        L = lib()
        assert L.frtm_backbone_set_bf16_pieces(self.bb, pieces) == 0 and L.frtm_backbone_set_bf16x1_3x3(self.bb, flag) == 0
        assert L.frtm_backbone_set_bf16_act(self.bb, act) == 0

    def shapes(self):
        """[(Cout, Cin, k, stride, pad)] in forward (index) order."""
        L, info, out = lib(), (ctypes.c_int * 6)(), []
        for i in range(L.frtm_backbone_num_convs(self.bb)):
            assert L.frtm_backbone_conv_info(self.bb, i, info) == 0
            out.append(tuple(info[:5]))
        return out

    def route(self, idx, B, hw):
        out3 = (ctypes.c_int * 3)()
        assert lib().frtm_backbone_conv_route(self.bb, idx, B, hw[0], hw[1], out3) == 0, lib().frtm_last_error()
        return tuple(out3)

    def plan(self, B, H, W):
        """frtm_backbone_act_plan: [(in, res, out)] per conv."""
        n = lib().frtm_backbone_num_convs(self.bb)
        buf = (ctypes.c_int * (3 * n))(*([-1] * (3 * n)))
        assert lib().frtm_backbone_act_plan(self.bb, B, H, W, buf, n) == 0, lib().frtm_last_error()
        return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]

    def blocks(self, H, W):
        """The block walk: a list of stages, each a list of blocks {'convs': [(idx, (Hin, Win))], 'ds': (idx, (Hin, Win)) or None, 'out_hw'}; conv indices
        in the order frtm_backbone_create numbers them (per block conv1 [conv2] [conv3] [downsample]), sizes from each conv's own geometry."""
        shapes = self.shapes()

        def out_hw(idx, hw):
            _, _, k, s, p = shapes[idx]
            return ((hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1)
        cur = out_hw(0, (H, W))                                              # the stem
        cur = ((cur[0] + 2 - 3) // 2 + 1, (cur[1] + 2 - 3) // 2 + 1)         # the 3x3 stride-2 pad-1 pool
        i, stages, inpl = 1, [], 64
        for s, nb in enumerate(BLOCKS[self.arch]):
            stage = []
            for b in range(nb):
                bl, hw = {'convs': [], 'ds': None}, cur
                for _ in range(3 if self.arch >= 50 else 2):
                    bl['convs'].append((i, hw))
                    hw = out_hw(i, hw)
                    i += 1
                cout = shapes[i - 1][0]
                if b == 0 and (s > 0 or cout != inpl):
                    assert shapes[i][2] == 1 and shapes[i][0] == cout and shapes[i][1] == inpl, shapes[i]
                    bl['ds'] = (i, cur)
                    i += 1
                bl['out_hw'] = cur = hw
                inpl = cout
                stage.append(bl)
            stages.append(stage)
        assert i == len(shapes)
        return stages

    def tensors(self, B, H, W):
        """Every tensor of the block walk that a conv writes: (producer idx, channels, [(reader idx, 'in' | 'res')], ends_stage)."""
        shapes, out = self.shapes(), []
        for stage in self.blocks(H, W):
            for b, bl in enumerate(stage):
                idxs = [i for i, _ in bl['convs']]
                for a, nxt in zip(idxs, idxs[1:]):                           # t1, t2
                    out.append((a, shapes[a][0], [(nxt, 'in')], False))
                if bl['ds']:
                    out.append((bl['ds'][0], shapes[bl['ds'][0]][0], [(idxs[-1], 'res')], False))
                readers = []
                if b + 1 < len(stage):
                    nx = stage[b + 1]
                    readers = [(nx['convs'][0][0], 'in')] + ([(nx['ds'][0], 'in')] if nx['ds'] else [(nx['convs'][-1][0], 'res')])
                out.append((idxs[-1], shapes[idxs[-1]][0], readers, b + 1 == len(stage)))
        return out

    def expected_plan(self, B, H, W, on):
        """The rule, tensor by tensor: bf16 exactly when the mode is in effect, C % 8 == 0, the tensor does not end a stage, and its producer and every
        reader are routed to layout 6, 7 or 8 at their own launch sizes (frtm_backbone_conv_route)."""
        sizes = {0: (H, W)}
        for stage in self.blocks(H, W):
            for bl in stage:
                sizes.update(dict(bl['convs'] + ([bl['ds']] if bl['ds'] else [])))
        routed = {i: self.route(i, B, hw)[0] in BF16_LAYOUTS for i, hw in sizes.items()}
        fmt = [[0, 0, 0] for _ in sizes]
        for prod, ch, readers, ends in self.tensors(B, H, W):
            bf = int(on and not ends and ch % 8 == 0 and routed[prod] and all(routed[r] for r, _ in readers))
            fmt[prod][2] = bf
            for r, how in readers:
                fmt[r][0 if how == 'in' else 1] = bf
        return [tuple(f) for f in fmt], routed, sizes
