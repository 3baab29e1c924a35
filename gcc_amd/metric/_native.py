"""What the native metric networks (drn_seg.DrnSegEngine, inception_fid.InceptionFidEngine) have in common: an evaluator whose
weights never change, run as a "slab program".

    construction   the state_dict is parsed on the host (conv_shape: the checks every conv + BatchNorm pair gets); the tensors the
                   network reads are kept as fp32 host copies
    .to(device)    every BatchNorm folded into a per-channel (scale, shift) by one BNEvalTable run, every weight packed: once
    a program      the launches of one input size as a list of step tuples over symbolic activations (Act) of ONE grow-only
                   slab: the input at its head, behind it four regions of the largest activation's size that the layers rotate
                   through.  An engine's _plan writes the program; _bind gives the activations their views of the slab and asks
                   the library about every conv geometry before anything runs.

An engine supplies BN_EPS, _pack (one conv's weights on the device), _plan (the program of a key whose first element is the batch
size), _conv (launch or route one 'conv' step), _declined (the refusal's text) and, if its slab is not bf16, _slab_dtype; its own
_run walks the steps."""
from types import SimpleNamespace

import torch

from .. import ops
from .._lib import GccError

BN_FIELDS = ('weight', 'bias', 'running_mean', 'running_var')


def _shape(v):
    return tuple(v.shape) if hasattr(v, 'shape') else tuple(v)


def conv_shape(sd, what, key, bn_prefix, kernel):
    """(co, ci) of the (kh, kw) convolution `key` of the state_dict sd (values: tensors, or bare shapes) with the BatchNorm
    `bn_prefix` behind it; raises GccError('<what>: ...') naming the first key that is missing or does not fit"""
    kh, kw = kernel
    if key not in sd:
        raise GccError('%s: %s is missing' % (what, key))
    s = _shape(sd[key])
    if len(s) != 4 or s[2:] != (kh, kw):
        raise GccError('%s: %s has shape %s, expected a %d x %d convolution' % (what, key, s, kh, kw))
    co, ci = s[0], s[1]
    if co % 8 or co <= 0:
        raise GccError('%s: %s has %d output channels; widths must be multiples of 8' % (what, key, co))
    fields = ['%s.%s' % (bn_prefix, f) for f in BN_FIELDS]
    for k in fields:
        if k not in sd:
            raise GccError('%s: %s is missing (BatchNorm behind %s)' % (what, k, key))
    for k in fields:
        if _shape(sd[k]) != (co,):
            raise GccError('%s: %s has shape %s, expected (%d,)' % (what, k, _shape(sd[k]), co))
    return co, ci


class Act:
    """symbolic activation of a program: C channels from `off` on in a pixel stride of ld, logical size h x w in phase layout d
    (drn_seg.py; 1: the logical layout), in slab region `region` (-1: the input, ahead of the regions); `view` once bound"""

    def __init__(self, C, h, w, region, d=1, ld=None, off=0):
        self.C, self.h, self.w, self.region, self.d, self.ld, self.off, self.view = C, h, w, region, d, ld or C, off, None


class SlabProgramEngine:
    BN_EPS = None                                        # a state_dict does not carry it
    _slab_dtype = torch.bfloat16

    def __init__(self, state_dict, convs, extra_keys=()):
        """convs: the network's convolutions in launch order (key, bn, co), each with the BatchNorm behind it"""
        self.convs = convs
        keys = set(c.key for c in convs) | set('%s.%s' % (c.bn, f) for c in convs for f in BN_FIELDS) | set(extra_keys)
        self.host = {k: state_dict[k].detach().to('cpu', torch.float32).contiguous() for k in keys}
        self.device = None
        self._slab, self._programs = None, {}

    @property
    def _name(self):
        return type(self).__name__

    # ---- host -> device: once -------------------------------------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise GccError('%s runs on the GPU only (asked for %s)' % (self._name, device))
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.device == device:
            return self
        self.device = device
        self._slab, self._programs = None, {}
        with torch.cuda.device(device):
            n = sum(c.co for c in self.convs)
            bn = torch.empty((4, n), dtype=torch.float32)
            off = 0
            for c in self.convs:
                for i, f in enumerate(BN_FIELDS):
                    bn[i, off:off + c.co] = self.host['%s.%s' % (c.bn, f)]
                off += c.co
            self._bn = bn.to(device)
            entries, off = [], 0
            for c in self.convs:
                g, b, rm, rv = (self._bn[i, off:off + c.co] for i in range(4))
                entries.append((SimpleNamespace(weight=g, bias=b, running_mean=rm, running_var=rv, eps=self.BN_EPS), None, c.co))
                off += c.co
                c.w = self._pack(c, self.host[c.key].to(device))
            self._table = ops.BNEvalTable(entries, device)
            self._table.run()                          # scale = gamma / sqrt(var + eps), shift = beta - mean scale, fp32
            for i, c in enumerate(self.convs):
                c.scale, c.shift = self._table.scale[i], self._table.shift[i]
            self._to_extra(device)
        return self

    def _pack(self, c, master):
        """the packing the library reads of conv c's fp32 [Co, Ci, KH, KW] master on the device: pack_weights' bf16 W"""
        return ops.pack_weights(master.contiguous(memory_format=torch.channels_last), want_w=True, want_wt=False)[0]

    def _to_extra(self, device):
        """whatever else the network reads on the device"""

    def eval(self):
        return self

    # ---- programs and the slab ------------------------------------------------------------------------------------------
    def _program(self, *key):
        prog = self._programs.get(key)
        if prog is None:
            prog = self._programs[key] = self._plan(*key)
        return prog

    def _bind(self, N, *rest):
        """the program of an input size with its views of the slab.  The slab only grows; when it is replaced, the programs bound
        to the old one are dropped with it (their views would keep it alive) and made again on their next use."""
        prog = self._program(N, *rest)
        if self._slab is None or self._slab.numel() < prog.total:
            self._slab, self._programs = None, {}
            self._slab = torch.zeros(prog.total, dtype=self._slab_dtype, device=self.device)
            prog = self._program(N, *rest)
        if prog.slab is self._slab:
            return prog
        slab = self._slab

        def view(a):
            if a.view is None:
                base = 0 if a.region < 0 else prog.size_in + a.region * prog.size_r
                nb, h, w = N * a.d * a.d, a.h // a.d, a.w // a.d
                a.view = slab[base:base + nb * h * w * a.ld].view(nb, h, w, a.ld).permute(0, 3, 1, 2)[:, a.off:a.off + a.C]
        for st in prog.steps:
            for a in st[1:]:
                if isinstance(a, Act):
                    view(a)
        view(prog.last)
        prog.x_in = prog.steps[0][2].view               # the first conv's source: 3 channels, ahead of the regions
        prog.slab = slab
        self._check_routes(prog)
        return prog

    def _check_routes(self, prog):
        """every conv geometry asked of the library before anything runs: a declined one names its layer; there is no other route"""
        for st in prog.steps:
            if st[0] == 'conv' and self._conv(st, route_only=True) < 0:
                raise GccError(self._declined(st))

    def _conv_error(self, st, e):
        """the library's error e of the 'conv' step st under its layer's name (raised by the run loops themselves: a call per
        conv less on the host)"""
        return GccError('%s: %s: %s' % (self._name, st[1].key, e))

    # ---- the front of a call ----------------------------------------------------------------------------------------------
    def _check_input(self, x, refuse_empty=False):
        if (not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32
                or (refuse_empty and 0 in x.shape)):
            raise GccError('%s: expected an NCHW fp32 [N, 3, H, W] tensor, got %s %s'
                           % (self._name, getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))

    def _check_device(self, x=None):
        if self.device is None:
            raise GccError('%s: .to(device) first' % self._name)
        if x is not None and x.device != self.device:
            raise GccError('%s: the input is on %s, the engine on %s' % (self._name, x.device, self.device))
