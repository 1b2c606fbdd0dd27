"""The Vis-MVSNet feature CNN `FeatExt` (reference code/utils/my_utils.py:499-708) as an inference module on the HIP kernels of csrc/featext.hip,
and `extract_features`, the per-scene feature pass of the reference's SceneDataset (scene_dataset.py:138-149).

The network (eval-mode BatchNorm, eps 1e-5; every convolution without bias; "block(c, s)" = BasicBlock: relu(bn2(conv2(relu(bn1(conv1_s(x))))) + r)
with r = x, or r = bn(conv1x1_s(x)) where the block changes width or stride):

    x [N,3,H,W] -> init_conv: relu(bn(conv5x5 stride 2, 3->16))                      at R x S = ceil(H/2) x ceil(W/2)
    enc 2d2_0:  block(32, 1), block(32, 1)   -> e0 [32]   at R x S
    enc 2d4_1:  block(64, 2), block(64, 1)   -> e1 [64]   at R/2 x S/2
    enc 2d8_2:  block(128, 2), block(128, 1) -> e2 [128]  at R/4 x S/4
    dec 2d16_3: deconv(128->64), conv3x3(cat(., e1): 128->64), block(64, 1)  -> o2 [64]  at R/2 x S/2
    dec 2d8_4:  deconv(64->32),  conv3x3(cat(., e0): 64->32),  block(32, 1)  -> o3 [32]  at R x S
    -> (final_conv_1(e2), final_conv_2(o2), final_conv_3(o3)), each a plain conv3x3 to 32 channels

deconv = ConvTranspose2d(3, stride 2, padding 1, output_padding 1).  The decoder concatenation needs 2 * (R/4) == R/2 and 2 * (R/2) == R, i.e. R and S
multiples of 4; other shapes raise ValueError (the reference fails in torch.cat).  The submodule and parameter names are the reference's, so
`load_state_dict` takes its checkpoint entries as they are.
"""
import ctypes as C
import pickle
from collections import OrderedDict

import torch
import torch.nn as nn

from ._lib import check, lib

# the layers in the order of the kernels' table (csrc/featext.hip::FX_LAYERS): (conv module path, BatchNorm module path or None)
_ENC = [('unet.enc_blocks.%s.0.conv1', 'unet.enc_blocks.%s.0.bn1'), ('unet.enc_blocks.%s.0.conv2', 'unet.enc_blocks.%s.0.bn2'),
        ('unet.enc_blocks.%s.0.downsample.0', 'unet.enc_blocks.%s.0.downsample.1'),
        ('unet.enc_blocks.%s.1.conv1', 'unet.enc_blocks.%s.1.bn1'), ('unet.enc_blocks.%s.1.conv2', 'unet.enc_blocks.%s.1.bn2')]
_DEC = [('unet.dec_blocks.%s.0', None), ('unet.dec_blocks.%s.1', None),
        ('unet.dec_blocks.%s.2.0.conv1', 'unet.dec_blocks.%s.2.0.bn1'), ('unet.dec_blocks.%s.2.0.conv2', 'unet.dec_blocks.%s.2.0.bn2')]
LAYERS = ([('init_conv.0', 'init_conv.1')]
          + [(c % s, b % s) for s in ('2d2_0', '2d4_1', '2d8_2') for c, b in _ENC]
          + [(c % s, b % s if b else None) for s in ('2d16_3', '2d8_4') for c, b in _DEC]
          + [('final_conv_1', None), ('final_conv_2', None), ('final_conv_3', None)])
STAGES = ['init_conv', 'enc 2d2_0', 'enc 2d4_1', 'enc 2d8_2', 'dec 2d16_3', 'dec 2d8_4', 'heads']


def output_hw(h, w):
    """-> (R, S) = the size of the finest feature map (final_conv_3) of an h x w input; ValueError where the network cannot run."""
    R, S = (h + 1) // 2, (w + 1) // 2
    if h < 1 or w < 1 or R % 4 or S % 4:
        raise ValueError('FeatExt needs ceil(H/2) and ceil(W/2) to be multiples of 4 (the decoder concatenation), got H=%d W=%d' % (h, w))
    return R, S


class NamedModules(nn.Module):
    """Children registered under given names (the reference's ListModule: names from the UNet's '<prefix><scale>_<index>' strings, or list
    positions), iterated in registration order."""

    def __init__(self, named):
        super().__init__()
        items = named.items() if isinstance(named, OrderedDict) else enumerate(named)
        for name, m in items:
            self.add_module(str(name), m if isinstance(m, nn.Module) else NamedModules(m))

    def __iter__(self):
        return iter(self._modules.values())

    def __len__(self):
        return len(self._modules)


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = (nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
                           if stride != 1 or cin != cout else None)
        self.stride = stride


def _stage(cin, cout, blocks, stride):
    return nn.Sequential(BasicBlock(cin, cout, stride), *[BasicBlock(cout, cout, 1) for _ in range(blocks - 1)])


class UNet(nn.Module):
    """The parameter tree of FeatExt's UNet(16, enc=2, dec=1, initial_scale=2, bottom=[], filters=[32, 64, 128], head=[], '2d')."""

    def __init__(self):
        super().__init__()
        self.bottom_blocks = NamedModules(OrderedDict())
        self.enc_blocks = NamedModules(OrderedDict([('2d2_0', _stage(16, 32, 2, 1)), ('2d4_1', _stage(32, 64, 2, 2)), ('2d8_2', _stage(64, 128, 2, 2))]))
        dec = OrderedDict()
        for name, cin, c in (('2d16_3', 128, 64), ('2d8_4', 64, 32)):
            dec[name] = [nn.ConvTranspose2d(cin, c, 3, 2, 1, 1, bias=False), nn.Conv2d(2 * c, c, 3, 1, 1, bias=False), _stage(c, c, 1, 1)]
        self.dec_blocks = NamedModules(dec)
        self.head_blocks = NamedModules(OrderedDict())


class FeatExt(nn.Module):
    """Vis-MVSNet's feature extractor, inference only, on the device.  forward(x[N,3,H,W] fp32 on the GPU, NCHW or channels-last) -> the
    reference's (final_conv_1(out1), final_conv_2(out2), final_conv_3(out3)) as channels-last tensors [N,32,R/4,S/4], [N,32,R/2,S/2], [N,32,R,S]
    (R, S = output_hw(H, W)), with eval-mode semantics whatever self.training says.  The folded weights are packed once per change of the
    parameters (on the first forward after it)."""

    def __init__(self):
        super().__init__()
        self.init_conv = nn.Sequential(nn.Conv2d(3, 16, 5, 2, 2, bias=False), nn.BatchNorm2d(16), nn.ReLU())
        self.unet = UNet()
        self.final_conv_1 = nn.Conv2d(128, 32, 3, 1, 1, bias=False)
        self.final_conv_2 = nn.Conv2d(64, 32, 3, 1, 1, bias=False)
        self.final_conv_3 = nn.Conv2d(32, 32, 3, 1, 1, bias=False)
        self._packed, self._key, self._ws = None, None, None

    @classmethod
    def from_checkpoint(cls, path, map_location='cpu', weights_only=True):
        """A Vis-MVSNet checkpoint: its 'state_dict' entries under 'module.feat_ext.' (my_utils.py:702-703).  weights_only=True unpickles
        tensors and plain containers only; a checkpoint that also holds other pickled objects (the reference loads it in full) needs
        weights_only=False, which runs arbitrary pickle code: for trusted files only."""
        try:
            ckpt = torch.load(path, map_location=map_location, weights_only=weights_only)
        except pickle.UnpicklingError as e:
            raise RuntimeError('%s holds pickled objects other than tensors and containers; if the file is trusted, load it with '
                               'weights_only=False (FeatExt.from_checkpoint / SceneDataset(feat_weights_only=False)): %s' % (path, e)) from e
        m = cls()
        m.load_state_dict({k[16:]: v for k, v in ckpt['state_dict'].items() if k.startswith('module.feat_ext')})
        return m

    def raw_params(self):
        """-> fp32 [mvsdf_featext_raw_floats()] on the parameters' device: per layer of LAYERS its weight, then its BatchNorm's weight, bias,
        running_mean, running_var."""
        mods = dict(self.named_modules())
        parts = []
        for conv, bn in LAYERS:
            parts.append(mods[conv].weight.detach().reshape(-1))
            if bn:
                b = mods[bn]
                parts += [b.weight.detach(), b.bias.detach(), b.running_mean, b.running_var]
        return torch.cat([p.float().reshape(-1) for p in parts])

    def _state_key(self):
        return tuple((t.data_ptr(), t._version, t.device) for t in list(self.parameters()) + list(self.buffers()))

    def packed(self):
        key = self._state_key()
        if self._packed is None or self._key != key:
            raw = self.raw_params()
            if not raw.is_cuda:
                raise RuntimeError('FeatExt runs on the GPU: move the module there first (.cuda())')
            assert raw.numel() == lib().mvsdf_featext_raw_floats(), 'FeatExt layer table does not match the library'
            nb = lib().mvsdf_featext_pack_bytes()
            buf = torch.empty(nb // 4, dtype=torch.float32, device=raw.device)
            check(lib().mvsdf_featext_pack(C.c_void_p(raw.data_ptr()), C.c_void_p(buf.data_ptr()), nb,
                                           C.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)), 'mvsdf_featext_pack')
            self._packed, self._key = buf, key
        return self._packed

    def _workspace(self, n, h, w, device):
        nb = lib().mvsdf_featext_workspace_bytes(n, h, w)
        if nb == 0:
            output_hw(h, w)
            raise ValueError('FeatExt: unsupported input shape %s' % ((n, 3, h, w),))
        if self._ws is None or self._ws.numel() * 4 < nb or self._ws.device != device:
            self._ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=device)
        return self._ws, nb

    def release_workspace(self):
        """Drop the cached activation workspace (about 864 bytes per finest-level pixel per image; it is reallocated on the next forward)."""
        self._ws = None

    def run(self, x, out1=None, out2=None, out3=None, stages=(0, len(STAGES))):
        """The kernels on x (NHWC-contiguous [N,H,W,3] fp32 on the device) into NHWC outputs (each may be None); stages: the [first, last) range
        of STAGES (the workspace carries the activations between calls)."""
        n, h, w, _ = x.shape
        ws, nb = self._workspace(n, h, w, x.device)
        p = self.packed()
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().mvsdf_featext_forward(vp(p), vp(x), n, h, w, vp(ws), nb, vp(out1), vp(out2), vp(out3), stages[0], stages[1],
                                          C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), 'mvsdf_featext_forward')

    @staticmethod
    def _nhwc_input(x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('FeatExt takes x[N,3,H,W], got %s' % (tuple(x.shape),))
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('FeatExt takes fp32 CUDA tensors')
        if x.requires_grad:
            raise NotImplementedError('FeatExt is inference only: the input requires grad')
        output_hw(x.shape[2], x.shape[3])
        return x.permute(0, 2, 3, 1).contiguous()

    def forward(self, x):
        xh = self._nhwc_input(x)
        n, h, w, _ = xh.shape
        R, S = output_hw(h, w)
        outs = [torch.empty((n, r, s, 32), dtype=torch.float32, device=x.device) for r, s in ((R // 4, S // 4), (R // 2, S // 2), (R, S))]
        self.run(xh, *outs)
        return tuple(o.permute(0, 3, 1, 2) for o in outs)


def extract_features(feat_ext, rgb_2xd, batch=20):
    """scene_dataset.py:138-149: element [2] of FeatExt for every view of rgb_2xd [V,3,H,W], batch views per call -> [V,32,R,S] fp32
    channels-last on the device (no host copy).  rgb_2xd may live on the host; each batch is moved to feat_ext's device."""
    dev = next(feat_ext.parameters()).device
    V, _, h, w = rgb_2xd.shape
    R, S = output_hw(h, w)
    out = torch.empty((V, R, S, 32), dtype=torch.float32, device=dev)
    for s in range(0, V, batch):
        x = FeatExt._nhwc_input(rgb_2xd[s:s + batch].to(dev, torch.float32))
        feat_ext.run(x, None, None, out[s:s + batch])
    return out.permute(0, 3, 1, 2)


def extract_pyramid(feat_ext, rgb_2xd, batch=20):
    """All three of FeatExt's maps for every view of rgb_2xd [V,3,H,W], batch views per call -> ([V,R/4,S/4,32], [V,R/2,S/2,32], [V,R,S,32]) fp32,
    channels-last in memory and in shape (what stereo.cascade_sweep takes, coarsest first), on the device.  The last is extract_features' output."""
    dev = next(feat_ext.parameters()).device
    V, _, h, w = rgb_2xd.shape
    R, S = output_hw(h, w)
    outs = [torch.empty((V, r, s, 32), dtype=torch.float32, device=dev) for r, s in ((R // 4, S // 4), (R // 2, S // 2), (R, S))]
    for s in range(0, V, batch):
        x = FeatExt._nhwc_input(rgb_2xd[s:s + batch].to(dev, torch.float32))
        feat_ext.run(x, *(o[s:s + batch] for o in outs))
    return tuple(outs)


def conv_layer(x, weight, bias=None, stride=1, res=None, relu=False, x2=None, transposed=False):
    """One layer of the kernels alone (tests, timing): Conv2d(k, stride, padding k // 2) over NCHW x (channels-last or not), or with
    transposed=True ConvTranspose2d(3, 2, 1, output_padding 1); x2: more input channels read after x's (a concatenation that is never formed);
    -> relu?(conv + bias + res) channels-last."""
    n, c1, h, w = x.shape
    c2 = x2.shape[1] if x2 is not None else 0
    cout = weight.shape[1] if transposed else weight.shape[0]
    k = weight.shape[-1]
    nb = lib().mvsdf_featext_layer_workspace_bytes(int(transposed), c1 + c2, cout, k, stride)
    if nb == 0:
        raise ValueError('conv_layer: unsupported layer (cin %d, cout %d, k %d, stride %d, transposed %s)' % (c1 + c2, cout, k, stride, transposed))
    ho, wo = ((2 * h, 2 * w) if transposed else ((h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous() if t is not None else None
    xs, x2s, rs = nhwc(x), nhwc(x2), nhwc(res)
    wt, bt = weight.detach().float().contiguous(), bias.detach().float().contiguous() if bias is not None else None
    ws = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib().mvsdf_featext_layer(int(transposed), vp(wt), vp(bt), cout, k, stride, vp(xs), c1, vp(x2s), c2, n, h, w, vp(rs), int(relu), vp(ws),
                                    nb, vp(out), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), 'mvsdf_featext_layer')
    return out.permute(0, 3, 1, 2)
