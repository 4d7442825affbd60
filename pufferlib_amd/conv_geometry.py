"""Host-side geometry of pufferlib.models.Convolutional (models.py:113-157) for any frame shape: what encode_observations does to
a uint8 frame — ``permute(0, 3, 1, 2)`` for channel-last frames, ``[:, :, ::d, ::d]``, then Conv2d(C,32,8,s4) / Conv2d(32,64,4,s2) /
Conv2d(64,64,3,s1), all valid padding — as the numbers the kernels of csrc/igemm.hip take: the three byte strides of the first
layer's loader (the permute and the downsample are strides, never copies), every layer's input / output size, the flatten width, the
pixel-slot counts of the dX phases and the largest frame chunk 32-bit element offsets allow.  Pure Python: no torch, no GPU."""

CONV_STACK = ((32, 8, 4), (64, 4, 2), (64, 3, 1))     # (out channels, kernel, stride) of the NatureCNN
OFFSET_LIMIT = 1 << 31                                # the kernels index every operand with 32-bit element offsets


def conv_out(size, kernel, stride):
    """Output length of a valid-padding convolution along one axis (0 when the kernel does not fit)."""
    return (size - kernel) // stride + 1 if size >= kernel else 0


def phase_slots(ih, iw, stride):
    """(HP, WP): pixel slots per frame of every dX phase (input pixels with equal (y mod S, x mod S)) = ceil(IH / S), ceil(IW / S)."""
    return (ih + stride - 1) // stride, (iw + stride - 1) // stride


def phase_pixels(ih, iw, stride, py, px):
    """Input pixels of phase (py, px) that exist: slots (yy, xx) with yy*S + py < IH and xx*S + px < IW."""
    rows = (ih - py + stride - 1) // stride if py < ih else 0
    cols = (iw - px + stride - 1) // stride if px < iw else 0
    return rows * cols


class ConvGeometry:
    """obs_shape: the env's single_observation_space.shape, (C, H, W) or — channels_last — (H, W, C)."""

    def __init__(self, obs_shape, channels_last=False, downsample=1):
        obs_shape = tuple(int(s) for s in obs_shape)
        if len(obs_shape) != 3 or min(obs_shape) < 1:
            raise ValueError(f'models.Convolutional reads 3-D uint8 frames, got shape {obs_shape}')
        d = int(downsample)
        if d < 1:
            raise ValueError(f'downsample must be >= 1 (got {downsample})')
        self.obs_shape, self.channels_last, self.downsample = obs_shape, bool(channels_last), d
        if channels_last:
            h, w, c = obs_shape
            self.sc, self.sy, self.sx = 1, d * w * c, d * c
        else:
            c, h, w = obs_shape
            self.sc, self.sy, self.sx = h * w, d * w, d
        self.channels, self.raw_h, self.raw_w = c, h, w
        self.frame_bytes = c * h * w
        self.ih, self.iw = (h + d - 1) // d, (w + d - 1) // d          # len(range(0, h, d))
        self.layers = []                                               # (IC, IH, IW, OC, OH, OW, K, K, S) per conv layer
        ic, ih, iw = c, self.ih, self.iw
        for oc, k, s in CONV_STACK:
            oh, ow = conv_out(ih, k, s), conv_out(iw, k, s)
            if oh < 1 or ow < 1:
                raise ValueError(f'frames of {self.ih} x {self.iw} pixels (shape {obs_shape}, downsample {d}) are too small for the conv stack')
            self.layers.append((ic, ih, iw, oc, oh, ow, k, k, s))
            ic, ih, iw = oc, oh, ow
        self.out_shape = (ic, ih, iw)                                  # what nn.Flatten sees (NCHW)
        self.flat_size = ic * ih * iw
        if (64 * c) % 16 != 0:
            raise ValueError('conv1 contracts over 64 * channels patch elements: a multiple of 16')
        # the word loader of mode 2 (channel-first frames, no downsample, patch runs of four aligned bytes) is what the Atari shape takes
        self.aligned_chw = (not channels_last) and d == 1 and w % 4 == 0 and (c * h * w) % 4 == 0

    def check_flat_size(self, flat_size):
        if int(flat_size) != self.flat_size:
            raise ValueError(f'models.Convolutional: flat_size {int(flat_size)} but the conv stack on frames of shape {self.obs_shape} '
                             f'(channels_last={self.channels_last}, downsample={self.downsample}) yields {self.out_shape[0]} x '
                             f'{self.out_shape[1]} x {self.out_shape[2]} = {self.flat_size}')

    def elements_per_frame(self):
        """The largest per-frame operand the kernels address: the raw frame (bytes) or a layer's activation (floats)."""
        m = self.frame_bytes
        for ic, ih, iw, oc, oh, ow, _, _, _ in self.layers:
            m = max(m, ic * ih * iw, oc * oh * ow)
        return m

    def max_chunk(self):
        """Frames per kernel batch such that (frames + 1) * elements_per_frame() stays below 2^31 (ig_check_a's bound)."""
        return max(1, (OFFSET_LIMIT - 1) // self.elements_per_frame() - 1)

    def activation_bytes_per_frame(self):
        """fp32 activations + their gradients kept for one frame of a chunk (a1 a2 a3 and d1 d2 d3) + the frame itself."""
        return self.frame_bytes + 8 * sum(oc * oh * ow for _, _, _, oc, oh, ow, _, _, _ in self.layers)

    def chunk_for(self, memory_bytes=None):
        """Frames per kernel batch: the 2^31 bound, and — given a memory budget — as many frames as keep their activations inside it."""
        n = self.max_chunk()
        if memory_bytes is not None:
            n = min(n, max(1, int(memory_bytes) // self.activation_bytes_per_frame()))
        return n


def default_obs_shape(framestack, channels_last=False):
    """Where nobody recorded the env's frame shape: the Atari one."""
    return (84, 84, int(framestack)) if channels_last else (int(framestack), 84, 84)


class ResnetGeometry:
    """pufferlib.models.ProcgenResnet (models.py:159-231) on channel-last uint8 frames (H, W, C): three ConvSequences of
    Conv2d(3x3, padding 1) -> max_pool2d(3, stride 2, padding 1) -> two residual blocks, widths (w, 2w, 2w).  `seqs` holds
    (IC, H, W, OC, PH, PW) per sequence: the conv keeps (H, W), the pool yields ((H+1)//2, (W+1)//2)."""

    def __init__(self, obs_shape, cnn_width=16):
        obs_shape = tuple(int(s) for s in obs_shape)
        if len(obs_shape) != 3 or min(obs_shape) < 1:
            raise ValueError(f'models.ProcgenResnet reads 3-D uint8 frames (H, W, C), got shape {obs_shape}')
        h, w, c = obs_shape
        self.obs_shape, self.cnn_width = obs_shape, int(cnn_width)
        self.channels, self.frame_bytes = c, h * w * c
        self.sc, self.sy, self.sx = 1, w * c, c                        # `permute(0, 3, 1, 2)` is a set of strides, never a copy
        self.seqs = []
        ic = c
        for oc in (self.cnn_width, 2 * self.cnn_width, 2 * self.cnn_width):
            ph, pw = (h + 1) // 2, (w + 1) // 2
            self.seqs.append((ic, h, w, oc, ph, pw))
            ic, h, w = oc, ph, pw
        self.out_shape = (ic, h, w)                                    # what nn.Flatten sees (NCHW)
        self.flat_size = ic * h * w

    def elements_per_frame(self):
        return max([self.frame_bytes] + [oc * h * w for _, h, w, oc, _, _ in self.seqs])

    def max_chunk(self):
        return max(1, (OFFSET_LIMIT - 1) // self.elements_per_frame() - 1)

    def activation_bytes_per_frame(self):
        """fp32 maps kept for one frame of a chunk: per sequence the pre-pool map and five block-sized maps, plus the gradients (one
        pre-pool sized, three block sized), plus the frame."""
        return self.frame_bytes + 4 * sum(2 * oc * h * w + 8 * oc * ph * pw for _, h, w, oc, ph, pw in self.seqs)

    def chunk_for(self, memory_bytes=None):
        n = self.max_chunk()
        if memory_bytes is not None:
            n = min(n, max(1, int(memory_bytes) // self.activation_bytes_per_frame()))
        return n
