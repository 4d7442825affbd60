"""IMPALA ResNet policy engine: pufferlib.models.ProcgenResnet (models.py:159-231) behind frameworks.cleanrl.Policy, one kernel launch
per layer on the fp32-MFMA implicit-GEMM kernels of csrc/igemm.hip — the route cnn.py takes for the NatureCNN.

  SameConv.forward / backward_dx / backward_dw    one 3 x 3 padding-1 convolution (operand mode 5; the first layer, on the uint8 frames,
                                                  mode 6) with the epilogue its place in a residual block asks for
  Engine.forward(frames)                          uint8 frames (H, W, C) -> hidden [n][mlp_width]
  Engine.backward(...)                            d loss / d (pre-ReLU hidden) -> every weight / bias gradient
  policy_step / update_from / update / clip_adam  cnn.Engine's own (heads, PPO loss, chunking, Adam)

Activations are NHWC f32.  Per ConvSequence the forward keeps what the backward reads: the pre-pool map `c`, the pooled map `p` (block
0's input), the conv0 pre-activations `t0`, `t1`, block 1's input `x1` and the output `x2` (the last sequence's x2 is stored after
Flatten's ReLU: nothing else reads it).  ReLU is never a pass of its own: a block's conv0 / conv1 apply it as they load (reserved
bit 0), the skip connection reads the same buffer without it, and the dX epilogues mask by the stored pre-activation.
Algorithmic work per frame at Procgen's (64, 64, 3): forward 2 * (4096*27*16 + 4*1024*144*16 + 1024*144*32 + 4*256*288*32 + 256*288*32
+ 4*64*288*32 + 2048*256) = 82.8 MFLOP."""
import ctypes as C

import torch

from . import _lib, cnn
from ._lib import EPI_BIAS, EPI_BIAS_ADD, EPI_BIAS_ADD_RELU, EPI_MASK, EPI_MASK_ADD, EPI_NONE, MODE_IM2COL_PAD, MODE_IM2COL_U8P, operand
from .cnn import LinearLayer


class SameConv:
    """Conv2d(IC, OC, 3, padding=1) on [n][H][W][IC] NHWC f32 (`relu_in`: on relu of it), or on uint8 frames (`strides` = (sc, sy, sx,
    frame_bytes))."""

    def __init__(self, weight, bias, h, w, device, relu_in=False, strides=None):
        oc, ic, kh, kw = weight.shape
        self.w, self.b = weight, bias
        self.IC, self.OC, self.H, self.W, self.KH = ic, oc, h, w, kh
        self.u8 = strides is not None
        self.strides = tuple(strides) if strides else (0,) * 4
        self.mode = MODE_IM2COL_U8P if self.u8 else MODE_IM2COL_PAD
        self.relu_in = 1 if relu_in else 0
        self.K = ic * kh * kw
        self.KR = (self.K + 15) // 16 * 16                    # the rows form contracts over whole 16-element slabs
        self.geom = (ic, h, w, oc, h, w, kh, kw, 1)
        self.geom_t = (oc, h, w, ic, h, w, kh, kw, 1)         # dX: the same product on dOut with the channel roles swapped
        self.w_fwd = torch.zeros(oc, self.KR, device=device)  # (columns K .. KR-1 stay zero)
        self.KT = oc * kh * kw
        self.w_dx = None if self.u8 else torch.empty(ic, self.KT, device=device)

    def pack(self):
        _lib.check(_lib.lib().pfa_cnn_pack_conv_same(_lib.ptr(self.w), C.byref(operand(0, self.w, 0, self.geom)), 1 if self.u8 else 0,
                                                     _lib.ptr(self.w_fwd), self.KR, _lib.ptr(self.w_dx), _lib.stream_handle()), 'pack_conv_same')

    def rows(self, n):
        return n * self.H * self.W

    def _in(self, x):
        return operand(self.mode, x, 0, self.geom, self.strides, self.relu_in)

    def forward(self, x, n, out, epi=EPI_BIAS, addend=None):
        """out [n*H*W][OC] = conv(x) + bias (epi 1), + addend (epi 4), relu of that (epi 5)."""
        _lib.check(_lib.lib().pfa_igemm_rows_add(C.byref(self._in(x)), self.rows(n), self.KR, _lib.ptr(self.w_fwd), self.KR, self.OC, _lib.ptr(out),
                                                 self.OC, epi, _lib.ptr(self.b), None, 0, _lib.ptr(addend), self.OC, _lib.stream_handle()), 'same_conv_forward')

    def backward_dx(self, dout, n, dx, mask=None, addend=None):
        """dx [n*H*W][IC] = conv_transpose(dout), zeroed where mask <= 0 (the ReLU this layer read through), + addend (the skip gradient)."""
        a = operand(MODE_IM2COL_PAD, dout, 0, self.geom_t)
        epi = EPI_NONE if mask is None else (EPI_MASK if addend is None else EPI_MASK_ADD)
        _lib.check(_lib.lib().pfa_igemm_rows_add(C.byref(a), self.rows(n), self.KT, _lib.ptr(self.w_dx), self.KT, self.IC, _lib.ptr(dx), self.IC, epi, None,
                                                 _lib.ptr(mask), self.IC, _lib.ptr(addend), self.IC, _lib.stream_handle()), 'same_conv_dx')

    def backward_dw(self, x, n, dout, gw, gb, accumulate, ws):
        """gw ([OC][IC][3][3]) (+)= dout^T im2col(x) (of relu(x) where the forward read that); gb (+)= column sums of dout."""
        _lib.check(_lib.lib().pfa_igemm_weights(C.byref(self._in(x)), self.rows(n), self.K, _lib.ptr(dout), self.OC, self.OC, _lib.ptr(gw),
                                                5 if self.u8 else 2, 1 if accumulate else 0, _lib.ptr(gb), _lib.ptr(ws), _lib.stream_handle()), 'same_conv_dw')

    def dw_workspace(self, n):
        return _lib.lib().pfa_igemm_weights_workspace_bytes(self.rows(n), self.K, self.OC)


def maxpool_forward(x, n, h, w, c, out):
    _lib.check(_lib.lib().pfa_maxpool3s2_forward(_lib.ptr(x), n, h, w, c, _lib.ptr(out), _lib.stream_handle()), 'maxpool_forward')


def maxpool_backward(x, out, dout, n, h, w, c, dx):
    _lib.check(_lib.lib().pfa_maxpool3s2_backward(_lib.ptr(x), _lib.ptr(out), _lib.ptr(dout), n, h, w, c, _lib.ptr(dx), _lib.stream_handle()), 'maxpool_backward')


class Sequence:
    """One ConvSequence: its five convolutions and (after Engine._alloc) its activation and gradient maps."""

    def __init__(self, views, prefix, ic, h, w, oc, ph, pw, device, strides):
        def conv(name, hh, ww, relu_in=False, st=None):
            return SameConv(views[f'{prefix}.{name}.weight'], views[f'{prefix}.{name}.bias'], hh, ww, device, relu_in, st)
        self.prefix, self.IC, self.H, self.W, self.OC, self.PH, self.PW = prefix, ic, h, w, oc, ph, pw
        self.conv = conv('conv', h, w, st=strides)
        self.b0c0, self.b0c1 = conv('res_block0.conv0', ph, pw, True), conv('res_block0.conv1', ph, pw, True)
        self.b1c0, self.b1c1 = conv('res_block1.conv0', ph, pw, True), conv('res_block1.conv1', ph, pw, True)
        self.convs = [self.conv, self.b0c0, self.b0c1, self.b1c0, self.b1c1]

    def alloc(self, n, device):
        big, small = (n * self.H * self.W, self.OC), (n * self.PH * self.PW, self.OC)
        self.c, self.gc = torch.empty(big, device=device), torch.empty(big, device=device)
        self.p, self.t0, self.x1, self.t1, self.x2 = (torch.empty(small, device=device) for _ in range(5))
        self.g0, self.g1, self.gt = (torch.empty(small, device=device) for _ in range(3))

    def forward(self, x, n, last):
        self.conv.forward(x, n, self.c)
        maxpool_forward(self.c, n, self.H, self.W, self.OC, self.p)
        self.b0c0.forward(self.p, n, self.t0)
        self.b0c1.forward(self.t0, n, self.x1, EPI_BIAS_ADD, self.p)
        self.b1c0.forward(self.x1, n, self.t1)
        self.b1c1.forward(self.t1, n, self.x2, EPI_BIAS_ADD_RELU if last else EPI_BIAS_ADD, self.x1)
        return self.x2

    def backward(self, x, n, gv, acc, ws, dx):
        """self.g0 holds d loss / d x2 on entry.  Leaves d / d x1 in g1, d / d p in g0, d / d c in gc and, unless this is the first
        sequence (dx None), d / d (this sequence's input) in `dx`."""
        def grads(name):
            return gv[f'{self.prefix}.{name}.weight'], gv[f'{self.prefix}.{name}.bias']
        self.b1c1.backward_dw(self.t1, n, self.g0, *grads('res_block1.conv1'), acc, ws)
        self.b1c1.backward_dx(self.g0, n, self.gt, mask=self.t1)
        self.b1c0.backward_dw(self.x1, n, self.gt, *grads('res_block1.conv0'), acc, ws)
        self.b1c0.backward_dx(self.gt, n, self.g1, mask=self.x1, addend=self.g0)
        self.b0c1.backward_dw(self.t0, n, self.g1, *grads('res_block0.conv1'), acc, ws)
        self.b0c1.backward_dx(self.g1, n, self.gt, mask=self.t0)
        self.b0c0.backward_dw(self.p, n, self.gt, *grads('res_block0.conv0'), acc, ws)
        self.b0c0.backward_dx(self.gt, n, self.g0, mask=self.p, addend=self.g1)
        maxpool_backward(self.c, self.p, self.g0, n, self.H, self.W, self.OC, self.gc)
        self.conv.backward_dw(x, n, self.gc, *grads('conv'), acc, ws)
        if dx is not None:
            self.conv.backward_dx(self.gc, n, dx)


class Engine(cnn.Engine):
    """Forward / update of the ResNet policy over a models.ResnetParams buffer.  `chunk` = frames per kernel batch (about 1.5 MB of
    maps per frame at Procgen's shape), clamped to what 32-bit element offsets and a quarter of the device memory allow."""
    CHUNK_CAP = 4096

    def _build_layers(self, geo):
        v, dev = self.cp.views, self.dev
        strides = (geo.sc, geo.sy, geo.sx, geo.frame_bytes)
        self.seqs = [Sequence(v, f'network.{i}', ic, h, w, oc, ph, pw, dev, strides if i == 0 else None)
                     for i, (ic, h, w, oc, ph, pw) in enumerate(geo.seqs)]
        self.fc = LinearLayer(v['network.5.weight'], v['network.5.bias'], True, geo.out_shape, dev)
        self.layers = [c for s in self.seqs for c in s.convs] + [self.fc]

    def _alloc_maps(self, n):
        for s in self.seqs:
            s.alloc(n, self.dev)

    def forward(self, frames, n):
        """frames uint8 [n][frame_bytes] (H, W, C order) -> self.h[:n] (hidden, post-ReLU); keeps every map a backward reads."""
        assert n <= self.chunk
        self.pack()
        x = frames
        for i, s in enumerate(self.seqs):
            x = s.forward(x, n, last=i == len(self.seqs) - 1)
        self.fc.forward(x, n, self.h)
        return self.h[:n]

    def backward(self, frames, m, dh_pre, gv, acc):
        """Back-propagate d loss / d (pre-ReLU hidden) [m][hidden] through Linear(flat, hidden) and the three sequences of the chunk whose
        forward just ran; weight / bias gradients into the views `gv` (accumulate = acc)."""
        last = self.seqs[-1]
        self.fc.backward_dw(last.x2, m, dh_pre, gv['network.5.weight'], gv['network.5.bias'], acc, self.ws)
        self.fc.backward_dx(dh_pre, m, last.x2, last.g0)          # masked by Flatten's ReLU (x2 is stored behind it)
        for i in range(len(self.seqs) - 1, -1, -1):
            s = self.seqs[i]
            s.backward(self.seqs[i - 1].x2 if i else frames, m, gv, acc, self.ws, self.seqs[i - 1].g0 if i else None)
