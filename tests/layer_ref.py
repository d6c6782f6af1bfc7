"""A plain reference of ONE layer of the launch list, for the layer taps.

torch only, device-agnostic, no project code and no library convolution: a convolution is a sum over the kernel's taps of
`x_pad[:, kh::s, kw::s, :] @ w[kh, kw]`, in float64 (the reference) or float32 (the yardstick).  A layer is described by
one dict of `DifEmbedder.op_describe()` and fed the very tensors the kernel read (`DifEmbedder.tap`): the ROOT tensors of
its x and res.  `conv_layer` returns what the kernel must have stored in the view windows of y and y2, and the magnitude
A~ the a-priori bounds are stated on.

Bounds (u = 2^-24; derivations: DESIGN 4l).  With A~ = |scale| conv(|x~|, |w|) + |shift| + |res| and K = KH KW Cin:
  direct f32 forms   B = (K + 8) u A~
  Winograd forms     B = (Cin + 16 + 8) u A~w,  A~w = |scale| |A^T| (sum_c |G g G^T| (|B^T| |x~| |B|)) |A| + |shift| + |res|
  split-bf16 tiers   B = (K u + eps_t) A~,  eps_3 = 2^-22 (six products kept), eps_2 = 3 * 2^-16 (three kept)
y2 = act2(y scale2 + shift2) is held to the same form on A~2 = |scale2| A~ + |shift2|.

The split-bf16 tiers are also held to the sum of the terms they keep (`conv_layer(..., bf_terms=t)`): every operand as t
bf16 planes by repeated round-to-nearest-even (bf_planes: what bf3_split and net.hip's f32_to_bf16_rne do, bit for bit), the
linear part the sum over the kept pairs of planes (BF_KEPT) of the sum over taps.  In float64 that is the SPLIT REFERENCE S --
what a kernel of the tier computes but for its float32 accumulation; the truncation the tier commits on purpose is on both
sides and leaves the comparison.  In float32, the products added in the kernel's order (32-channel slice, tap, 16-channel half,
pair), it is the yardstick.  Against S:
  hard, per element  |y - S| <= (NQ K M + 8) u A~,  NQ = 6 / 3 products per multiply-add, M = 1 + 2^-6 + 2^-13 (BF_MAG: the planes'
                     absolute values add up to at most (1 + 2^-7 + 2^-16) |x|, for both operands)
  tight, max         max |y - S| / A~ <= 8 max(yardstick's, 2 u)
  tight, rms         rms((y - S) / A~) <= RMS_MARGIN x the yardstick's rms: the statistic that tells the tiers apart

The heads and NN4's own layers return (ref, B), B elementwise and stated on what was summed:
  dwfull             B = (HW + 8) u A~,  A~ = |scale| sum |x| |w| + |beta| + |mean scale|  (the shift by its parts, as dwconv_layer)
  gdc tail           the bound propagated stage by stage through depthwise, 1x1, dense and the normalisation (gdc_tail_layer)
  l2norm             B = (D / 2 + 4) u |ref|
  lrn                B = (P + 12) u |ref|,  P = POWF_ULP
  pool l2 / avg      B = (k^2 + 4) u |ref|  /  (k^2 + 2) u sum |x| / k^2;  max stays bit-exact
The worst-case chain of the tail is loose (a float32 run sits at 1e-4 of it), so these also pass the tight gate in units of B
(gate_in_B): max |y - ref| / B <= 8 max(max |y32 - ref| / B, max 2 u |ref| / B), y32 the same layer in float32.
"""
import torch

U = 2.0 ** -24
EPS_BF3 = 2.0 ** -22          # hi.hi + hi.mid + mid.hi + mid.mid + hi.lo + lo.hi kept; mid.lo, lo.mid, lo.lo and both residuals dropped
EPS_BF2 = 3 * 2.0 ** -16      # hi.hi + hi.mid + mid.hi kept; mid.mid and the two residuals (2^-16 each) dropped
# the kept products as (activation plane, weight plane), 0 = hi, 1 = mid, 2 = lo, in the order conv_bf_mainloop.hpp issues
# them per 16 k (small terms first)
BF_KEPT = {3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)), 2: ((1, 0), (0, 1), (0, 0))}
BF_MAG = 1 + 2.0 ** -6 + 2.0 ** -13   # sum over kept pairs of |x_p| |w_q| <= (1 + 2^-7 + 2^-16)^2 |x| |w| < BF_MAG |x| |w|
BF_SLICE, BF_HALF = 32, 16    # the mainloop's K order: 32-channel slices, nine taps each, two 16-channel MFMAs a tap
# rms((y - S) / A~) of a kernel over that of the float32 yardstick.  Above 1: another order of summation (MFMA sums of 16,
# stream-K shares).  Below the smallest ratio a lost plane leaves on the layers of tests/test_layer_ref.py (mid.mid dropped
# everywhere at K = 4608: x 4.43; every lo product dropped: x 5.56; at K = 576 x 10.4 and x 12.7 -- the table
# test_split_gates_planted_defects prints): the geometric middle of 1 and 4.43.
RMS_MARGIN = 2.1
CHUNK_ELEMS = 1 << 26         # elements of one padded input chunk (images are independent: the sum over taps is chunked)


class NotUnderstood(Exception):
    """A describe line holds something this reference does not model: the caller fails, it does not skip."""


def act(v, kind, alpha=None):
    if kind == 'none':
        return v
    if kind == 'relu':
        return v.clamp_min(0)
    if kind == 'relu6':
        return v.clamp(0, 6)
    if kind == 'prelu':
        return torch.where(v >= 0, v, v * alpha)
    raise NotUnderstood('activation %r' % (kind,))


def _p(params, name, like):
    return torch.as_tensor(params[name]).to(device=like.device, dtype=like.dtype)


def fold(params, bn, bias, C, like):
    """scale, shift of `(acc + bias) -> BN` from the raw parameters, in like's dtype: scale = gamma / sqrt(var + eps),
    shift = beta - mean scale + bias scale; no BN: scale 1, shift = bias."""
    scale = torch.ones(C, dtype=like.dtype, device=like.device)
    shift = torch.zeros(C, dtype=like.dtype, device=like.device)
    if bn is not None:
        prefix, eps = bn
        scale = _p(params, prefix + '/gamma', like) / torch.sqrt(_p(params, prefix + '/moving_variance', like) + eps)
        shift = _p(params, prefix + '/beta', like) - _p(params, prefix + '/moving_mean', like) * scale
        if bias is not None:
            shift = shift + _p(params, bias, like) * scale
    elif bias is not None:
        shift = _p(params, bias, like).clone()
    return scale, shift


def _whole(t, what):
    if t['coff'] or t['oy'] or t['ox'] or t['view'][:2] != t['root'][:2]:
        raise NotUnderstood('%s is a window of its root: %r' % (what, t))


def geometry(desc):
    """(Ho, Wo) of the convolution / pool: the first output's view, or the second's where the first keeps its even pixels."""
    t = desc['y2'] if (desc['y'] is None or desc.get('y_sub')) else desc['y']
    return t['view'][0], t['view'][1]


def kernel_hwio(desc, params, like):
    """The layer's weights as [KH, KW, Cin_true, Cout]: Keras HWIO, or a dense kernel [in, out] whose rows run over
    (h, w, c) -- after a channel-major flatten (chw_flatten) over (c, h, w)."""
    KH, KW = desc['k']
    ci, co = desc['cin_true'], desc['cout']
    w = _p(params, desc['w'], like)
    if w.numel() != KH * KW * ci * co:
        raise NotUnderstood('weight %s has %d elements for %dx%dx%dx%d' % (desc['w'], w.numel(), KH, KW, ci, co))
    if desc['chw_flatten']:
        return w.reshape(ci, KH, KW, co).permute(1, 2, 0, 3).contiguous()
    return w.reshape(KH, KW, ci, co)


def taps_sum(x, w, stride, pad_t, pad_l, Ho, Wo):
    """sum over taps of x_pad[:, kh::s, kw::s, :] @ w[kh, kw] -> [n, Ho, Wo, Cout]; zeros outside the map on every side the
    output geometry reaches (asymmetric padding: top / left as given, bottom / right as far as Ho, Wo need)."""
    n, H, W, C = x.shape
    KH, KW = w.shape[:2]
    pb = max((Ho - 1) * stride + KH - H - pad_t, 0)
    pr = max((Wo - 1) * stride + KW - W - pad_l, 0)
    out = torch.empty((n, Ho, Wo, w.shape[3]), dtype=x.dtype, device=x.device)
    per = (H + pad_t + pb) * (W + pad_l + pr) * max(C, w.shape[3])
    step = max(1, CHUNK_ELEMS // per)
    for s in range(0, n, step):
        xp = torch.nn.functional.pad(x[s:s + step], (0, 0, pad_l, pr, pad_t, pb))
        acc = None
        for kh in range(KH):
            for kw in range(KW):
                win = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :]
                t = win.reshape(-1, C) @ w[kh, kw]
                acc = t if acc is None else acc + t
        out[s:s + step] = acc.reshape(-1, Ho, Wo, w.shape[3])
    return out


# ----------------------------------------------------------------------------------------------- split-bf16
def bf_planes(t, n):
    """A float32 tensor as n bf16-valued float32 planes by repeated round-to-nearest-even: hi = bf16(t), mid = bf16(t - hi),
    lo = bf16(t - hi - mid) (gemm_core.hpp: bf3_split on the activations, net.hip: f32_to_bf16_rne on the HWIO kernel).  Each
    remainder is exact in float32."""
    if t.dtype != torch.float32:
        raise NotUnderstood('bf_planes of a %s tensor: the kernels split float32 operands' % (t.dtype,))
    out, r = [], t
    for _ in range(n):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p
    return out


def split_taps_sum(xp, wp, pairs, stride, pad_t, pad_l, Ho, Wo, kernel_order=False):
    """sum over the kept (p, q) of taps_sum(xp[p], wp[q]) in the planes' dtype.  kernel_order: product by product as
    gemm_mainloop_patch_bf3 / _bf2t add them into ONE accumulator -- per 32-channel slice the taps row by row, per tap two halves
    of 16 channels, per half the pairs in BF_KEPT's order (the float32 yardstick); otherwise pair by pair (float64: the order is
    immaterial at 2^-53)."""
    if not kernel_order:
        acc = None
        for p, q in pairs:
            t = taps_sum(xp[p], wp[q], stride, pad_t, pad_l, Ho, Wo)
            acc = t if acc is None else acc + t
        return acc
    n, H, W, C = xp[0].shape
    KH, KW, _, co = wp[0].shape
    pb = max((Ho - 1) * stride + KH - H - pad_t, 0)
    pr = max((Wo - 1) * stride + KW - W - pad_l, 0)
    out = torch.empty((n, Ho, Wo, co), dtype=xp[0].dtype, device=xp[0].device)
    per = len(xp) * (H + pad_t + pb) * (W + pad_l + pr) * max(C, co)
    step = max(1, CHUNK_ELEMS // per)
    for s in range(0, n, step):
        pads = [torch.nn.functional.pad(x[s:s + step], (0, 0, pad_l, pr, pad_t, pb)) for x in xp]
        acc = torch.zeros((pads[0].shape[0] * Ho * Wo, co), dtype=out.dtype, device=out.device)
        for c0 in range(0, C, BF_SLICE):
            for kh in range(KH):
                for kw in range(KW):
                    wins = [t[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, c0:c0 + BF_SLICE].reshape(-1, min(BF_SLICE, C - c0))
                            for t in pads]
                    for h0 in range(0, wins[0].shape[1], BF_HALF):
                        for p, q in pairs:
                            acc = acc + wins[p][:, h0:h0 + BF_HALF] @ wp[q][kh, kw, c0 + h0:c0 + h0 + BF_HALF]
        out[s:s + step] = acc.reshape(-1, Ho, Wo, co)
    return out


# ----------------------------------------------------------------------------------------------- Winograd F(2x2,3x3)
_G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]


def _bt(a, axis, absolute):
    x0, x1, x2, x3 = a.unbind(axis)
    if absolute:
        return torch.stack([x0 + x2, x1 + x2, x2 + x1, x1 + x3], axis)
    return torch.stack([x0 - x2, x1 + x2, x2 - x1, x1 - x3], axis)


def wino_even(x, w, absolute=False):
    """The Winograd kernels' order of operations on an even map (a torch port of tools/winograd_error.py: wino_even):
    U = G g G^T in float64 rounded once to x's dtype, V = B^T d B, sixteen products summed over Cin, Y = A^T M A, all in x's
    dtype.  absolute: every matrix and operand by its absolute value -- the magnitude the rounding bound is stated on."""
    n, H, W, C = x.shape
    co = w.shape[3]
    G = torch.tensor(_G, dtype=torch.float64, device=x.device)
    u = torch.einsum('ik,klco,jl->ijco', G, w.to(torch.float64), G)
    if absolute:
        u = u.abs()
    u = u.to(x.dtype)
    th, tw = H // 2, W // 2
    out = torch.empty((n, H, W, co), dtype=x.dtype, device=x.device)
    step = max(1, CHUNK_ELEMS // (4 * (H + 2) * (W + 2) * max(C, co)))
    sg = 1 if absolute else -1
    for s in range(0, n, step):
        xp = torch.nn.functional.pad(x[s:s + step], (0, 0, 1, 1, 1, 1))
        d = torch.stack([torch.stack([xp[:, r:r + 2 * th:2, c:c + 2 * tw:2, :] for c in range(4)], 3) for r in range(4)], 3)
        v = _bt(_bt(d, 3, absolute), 4, absolute)                       # [n, th, tw, 4, 4, C]
        m = torch.einsum('ntsijc,ijco->ntsijo', v, u)
        s0 = m[:, :, :, 0] + m[:, :, :, 1] + m[:, :, :, 2]
        s1 = m[:, :, :, 1] + sg * m[:, :, :, 2] + sg * m[:, :, :, 3]
        y = torch.empty((m.shape[0], th, 2, tw, 2, co), dtype=x.dtype, device=x.device)
        for a, t in enumerate((s0, s1)):
            y[:, :, a, :, 0] = t[:, :, :, 0] + t[:, :, :, 1] + t[:, :, :, 2]
            y[:, :, a, :, 1] = t[:, :, :, 1] + sg * t[:, :, :, 2] + sg * t[:, :, :, 3]
        out[s:s + step] = y.reshape(-1, H, W, co)
    return out


def wino_any(x, w, absolute=False):
    """... on any map: an odd side is zero-padded to even and cropped, as the kernel's out-of-range loads and masked stores do."""
    H, W = x.shape[1:3]
    if H % 2 or W % 2:
        return wino_even(torch.nn.functional.pad(x, (0, 0, 0, W % 2, 0, H % 2)), w, absolute)[:, :H, :W]
    return wino_even(x, w, absolute)


# ----------------------------------------------------------------------------------------------- the convolution layer
def window(t, root):
    """The view window of a root tensor [n, H, W, C]."""
    h, w, c = t['view']
    return root[:, t['oy']:t['oy'] + h, t['ox']:t['ox'] + w, t['coff']:t['coff'] + c]


def conv_layer(desc, params, x, res=None, dtype=torch.float64, form='direct', bf_terms=0):
    """One OP_CONV launch.  x, res: the ROOT tensors the kernel read ([n, H, W, C], any float dtype).  Returns (y, y2, A, A2)
    shaped as the layer's output map [n, Ho, Wo, Cout] (None where the layer has no such output; `stored(desc, ...)` cuts them
    to what the kernel stores): in `dtype`, in the fused order the kernels document (conv_splitk.hpp: SkEpi / conv_epilogue)
        x~ = pre_act(pre_bn(x));  v = conv(x~, w);  y = act(v scale + shift) (+ res at res_stride);  y2 = act2(y scale2 + shift2)
    and the magnitudes A = |scale| conv(|x~|, |w|) + |shift| + |res|, A2 = |scale2| A + |shift2|.
    form 'direct' sums the taps; 'wino' runs the Winograd kernels' order of operations (the float32 yardstick) and takes A
    through the transforms in absolute value.
    bf_terms 3 / 2 (form 'direct'): the linear part is the sum over BF_KEPT[bf_terms] of the tap sums of the bf16 planes of
    x~ and of the HWIO kernel, both split from their float32 values -- in float64 the split reference, in float32 and in the
    kernel's order of products the yardstick of the split-bf16 tiers.  Everything else, A included, is untouched."""
    if desc['kind'] != 'conv':
        raise NotUnderstood('conv_layer on %r' % desc['kind'])
    _whole(desc['x'], 'x')
    KH, KW = desc['k']
    Ho, Wo = geometry(desc)
    ci, co = desc['cin_true'], desc['cout']
    if desc['x']['root'][2] != desc['cin'] or ci > desc['cin']:
        raise NotUnderstood('x has %d channels, cin %d / %d' % (desc['x']['root'][2], desc['cin'], ci))
    xt = x[..., :ci].to(dtype)
    if desc['pre_bn'] is not None:
        ps, psh = fold(params, desc['pre_bn'], None, ci, xt)
        xt = act(xt * ps + psh, desc['pre_act'])
    elif desc['pre_act'] != 'none':
        raise NotUnderstood('pre_act without pre_bn')
    w = kernel_hwio(desc, params, xt)
    scale, shift = fold(params, desc['bn'], desc['bias'], co, xt)
    if form == 'wino':
        if (KH, KW, desc['stride']) != (3, 3, 1) or desc['pad'] != (1, 1) or (Ho, Wo) != tuple(xt.shape[1:3]):
            raise NotUnderstood('Winograd form on %r' % (desc,))
        # the reference proper stays the plain sum over taps; the yardstick (any narrower dtype) takes the kernels' order
        v = wino_any(xt, w) if dtype != torch.float64 else taps_sum(xt, w, 1, 1, 1, Ho, Wo)
        mag = wino_any(xt.abs(), w, absolute=True)
    elif bf_terms:
        if bf_terms not in BF_KEPT or form not in ('direct', 'bf16'):
            raise NotUnderstood('%r bf16 terms in form %r' % (bf_terms, form))
        # the kernel splits the float32 values it holds: x~ formed in float32 (today no split-bf16 layer has a pre_bn: x~ = x),
        # the kernel as the parameters store it
        xp = [t.to(dtype) for t in bf_planes(xt.to(torch.float32), bf_terms)]
        wp = [t.to(dtype) for t in bf_planes(kernel_hwio(desc, params, xt.to(torch.float32)), bf_terms)]
        v = split_taps_sum(xp, wp, BF_KEPT[bf_terms], desc['stride'], desc['pad'][0], desc['pad'][1], Ho, Wo, dtype != torch.float64)
        mag = taps_sum(xt.abs(), w.abs(), desc['stride'], desc['pad'][0], desc['pad'][1], Ho, Wo)
    else:
        v = taps_sum(xt, w, desc['stride'], desc['pad'][0], desc['pad'][1], Ho, Wo)
        mag = taps_sum(xt.abs(), w.abs(), desc['stride'], desc['pad'][0], desc['pad'][1], Ho, Wo)
    alpha = None
    if desc['act'] == 'prelu':
        alpha = _p(params, desc['alpha'], xt) if desc['alpha'] else torch.full((co,), desc['const_alpha'], dtype=dtype, device=xt.device)
    y = act(v * scale + shift, desc['act'], alpha)
    A = mag * scale.abs() + shift.abs()
    if desc['res'] is not None:
        _whole(desc['res'], 'res')
        rs = desc['res_stride']
        r = res.to(dtype)[:, ::rs, ::rs, :][:, :Ho, :Wo, :]
        if r.shape != y.shape:
            raise NotUnderstood('shortcut %s for output %s' % (tuple(r.shape), tuple(y.shape)))
        y = y + r
        A = A + r.abs()
    y2 = A2 = None
    if desc['y2'] is not None:
        s2, sh2 = fold(params, desc['bn2'], None, co, xt)
        y2 = act(y * s2 + sh2, desc['act2'], _p(params, desc['alpha2'], xt) if desc['alpha2'] else None)
        A2 = A * s2.abs() + sh2.abs()
    if desc['y'] is None:
        y = None
    return y, y2, A, A2


def stored(desc, key, full):
    """What the kernel stores of an output map: its even pixels for a sub-sampled first output."""
    return full[:, ::2, ::2, :] if (key == 'y' and desc.get('y_sub')) else full


def bound_factor(desc, form, bf_terms=0):
    """B / A~ for this layer and kernel form ('direct', 'wino', 'bf16')."""
    KH, KW = desc['k']
    if form == 'wino':
        return (desc['cin'] + 16 + 8) * U
    K = KH * KW * desc['cin_true']
    if form == 'bf16':
        return K * U + (EPS_BF3 if bf_terms == 3 else EPS_BF2)
    return (K + 8) * U


def split_bound_factor(desc, bf_terms):
    """B / A~ of a split-bf16 tier against its split reference: NQ K products in one float32 sum of magnitude <= BF_MAG A~."""
    KH, KW = desc['k']
    return (len(BF_KEPT[bf_terms]) * KH * KW * desc['cin_true'] * BF_MAG + 8) * U


# ----------------------------------------------------------------------------------------------- the exact layers
def input_convert(x, layout_nchw, scale, bias, bgr=False, hflip=False):
    """input_convert_kernel: [n,H,W,3] or [n,3,H,W], uint8 or float32 -> float32 [n,H,W,4], channel 3 zero,
    y[c] = x[2 - c if bgr else c] * scale + bias[c] as one fused multiply-add (float64 here, rounded once)."""
    t = x.permute(0, 2, 3, 1) if layout_nchw else x
    t = t.to(torch.float64)
    if hflip:
        t = t.flip(2)
    if bgr:
        t = t.flip(3)
    s = torch.tensor(scale, dtype=torch.float32).to(torch.float64)
    b = torch.tensor(list(bias), dtype=torch.float32).to(device=t.device, dtype=torch.float64)
    y = (t * s + b).to(torch.float32)
    return torch.nn.functional.pad(y, (0, 1))


def pool_layer(desc, params, x, dtype=torch.float64):
    """maxpool_kernel -> (y, y2, B).  Taps outside the map are skipped in every mode; windows may hang over the bottom /
    right edge (ceil).
    'max': exact (B None), skipped taps are -inf, or count as 0 with zero_pad; y2 = act2(fma(y, scale2, shift2)) in float32.
    'l2':  sqrt((sum_taps x^2 (1 / k^2)) k^2) -- the divisor is k^2 whatever the window holds, and is multiplied back.
           B = (k^2 + 4) u |ref|: k^2 fused terms, the two scalings, and the root.
    'avg': (sum_taps x) (1 / k^2).  B = (k^2 + 2) u sum |x| / k^2.
    A zero tap adds nothing to either sum, so zero_pad changes nothing there.  x float32 ('max') or any float dtype."""
    mode = desc['pool']
    if mode not in ('max', 'l2', 'avg'):
        raise NotUnderstood('pool mode %r' % mode)
    _whole(desc['x'], 'x')
    k, s = desc['k'][0], desc['stride']
    if desc['k'][1] != k:
        raise NotUnderstood('pool window %r' % (desc['k'],))
    pt, pl = desc['pad']
    Ho, Wo = desc['y']['view'][:2]
    n, H, W, C = x.shape
    pb = max((Ho - 1) * s + k - H - pt, 0)
    pr = max((Wo - 1) * s + k - W - pl, 0)
    if mode != 'max':
        if desc['y2'] is not None:
            raise NotUnderstood('a second output on an %s pool: the library builds none' % mode)
        xp = torch.nn.functional.pad(x.to(dtype), (0, 0, pl, pr, pt, pb))
        acc = torch.zeros((n, Ho, Wo, C), dtype=dtype, device=x.device)
        mag = torch.zeros((n, Ho, Wo, C), dtype=torch.float64, device=x.device)
        for kh in range(k):
            for kw in range(k):
                win = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :]
                acc = acc + (win * win if mode == 'l2' else win)
                mag = mag + win.abs().to(torch.float64)
        inv = torch.tensor(1.0 / (k * k), dtype=dtype, device=x.device)            # rounded in the yardstick as in the kernel
        if mode == 'l2':
            y = torch.sqrt((acc * inv) * (k * k))
            return y, None, (k * k + 4) * U * y.abs().to(torch.float64)
        y = acc * inv
        return y, None, (k * k + 2) * U * mag / (k * k)
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb), value=0.0 if desc['zero_pad'] else float('-inf'))
    y = None
    for kh in range(k):
        for kw in range(k):
            win = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :]
            y = win if y is None else torch.maximum(y, win)
    y2 = None
    if desc['y2'] is not None:
        one = torch.ones(C, dtype=torch.float32, device=x.device)
        s2, sh2 = fold32(params, desc['bn2'], C, x.device) if desc['bn2'] is not None else (one, 0 * one)
        y2 = act((y.to(torch.float64) * s2.to(torch.float64) + sh2.to(torch.float64)).to(torch.float32), desc['act2'])
    return y, y2, None


def fold32(params, bn, C, device):
    """The library's own float32 fold (net.hip: fold), operation by operation and on the host, as the library does it: an
    exact layer needs the exact constants."""
    import numpy as np
    prefix, eps = bn
    g, b, m, v = (np.asarray(params[prefix + '/' + k], np.float32) for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    sc = (g / np.sqrt(v + np.float32(eps))).astype(np.float32)
    sh = (b - (m * sc).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(sc).to(device), torch.from_numpy(sh).to(device)


def upsample_layer(x):
    """upsample2_kernel: nearest neighbour x 2."""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def dwconv_layer(desc, params, x, dtype=torch.float64):
    """dwconv_kernel: y = act((sum_taps x w[tap][c]) scale + shift), w [K, K, C, 1].  Returns (y, A) with
    A = |scale| sum |x| |w| + |beta| + |mean scale|: the shift enters by the magnitude of the PARTS it is folded from.  The
    library folds in float32, so shift carries u (|beta| + |mean scale|) whatever is left of it after the subtraction, and
    a depthwise window of a ReLU6 map is often all zero: there |shift| alone is the whole magnitude, and where beta and
    mean scale cancel (MobileNetV2's synthetic block_7_depthwise_BN channel 326: 0.082069 - 0.082066) the fold's rounding
    is 3 000 x (K + 8) u |shift|.  Measured on the MI355X before this was taken into A."""
    _whole(desc['x'], 'x')
    K, s = desc['k'][0], desc['stride']
    pt, pl = desc['pad']
    Ho, Wo = desc['y']['view'][:2]
    xt = x.to(dtype)
    n, H, W, C = xt.shape
    w = _p(params, desc['w'], xt).reshape(K, K, C)
    scale, shift = fold(params, desc['bn'], None, C, xt)
    pb = max((Ho - 1) * s + K - H - pt, 0)
    pr = max((Wo - 1) * s + K - W - pl, 0)
    xp = torch.nn.functional.pad(xt, (0, 0, pl, pr, pt, pb))
    v = torch.zeros((n, Ho, Wo, C), dtype=dtype, device=xt.device)
    mag = torch.zeros_like(v)
    for kh in range(K):
        for kw in range(K):
            win = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :]
            v += win * w[kh, kw]
            mag += win.abs() * w[kh, kw].abs()
    parts = shift.abs()
    if desc['bn'] is not None:
        parts = _p(params, desc['bn'][0] + '/beta', xt).abs() + (_p(params, desc['bn'][0] + '/moving_mean', xt) * scale).abs()
    return act(v * scale + shift, desc['act']), mag * scale.abs() + parts


# ----------------------------------------------------------------------------------------------- heads, LRN
L2_EPS = 1e-12                # l2norm_kernel / gdc_tail_*: x rsqrt(max(sum x^2, 1e-12)), as the kernels document
# The maximum ULP error of the device powf.  The toolchain ships no copy of the HIP math-API accuracy table, so this is the
# OpenCL limit for pow the device library is built to (OpenCL C 3.0, 7.4: pow <= 16 ulp) -- not read off the kernel's output.
POWF_ULP = 16


def _depthwise_full(desc, params, x, dtype):
    """a = (sum_p x[p, c] w[p, c]) scale + shift over the whole map, and A~ = |scale| sum |x| |w| + |beta| + |mean scale|
    (float64) -- the shift by the parts it is folded from, as dwconv_layer and for its reason."""
    _whole(desc['x'], 'x')
    xt = x.to(dtype)
    n, H, W, C = xt.shape
    if desc['k'] != (H, W):
        raise NotUnderstood('depthwise kernel %r on a %d x %d map' % (desc['k'], H, W))
    w = _p(params, desc['w'], xt).reshape(H * W, C)
    scale, shift = fold(params, desc['bn'], None, C, xt)
    xr = xt.reshape(n, H * W, C)
    a = (xr * w).sum(1) * scale + shift
    x64, w64 = xr.to(torch.float64), w.to(torch.float64)
    s64, sh64 = fold(params, desc['bn'], None, C, x64)
    parts = sh64.abs()
    if desc['bn'] is not None:
        parts = _p(params, desc['bn'][0] + '/beta', x64).abs() + (_p(params, desc['bn'][0] + '/moving_mean', x64) * s64).abs()
    return a, (x64.abs() * w64.abs()).sum(1) * s64.abs() + parts


def dwfull_layer(desc, params, x, dtype=torch.float64):
    """dwfull_kernel: the depthwise convolution whose kernel is the whole map, + BN -> ([n, 1, 1, C], B = (HW + 8) u A~)."""
    a, A = _depthwise_full(desc, params, x, dtype)
    n, C = a.shape
    HW = desc['k'][0] * desc['k'][1]
    return a.reshape(n, 1, 1, C), ((HW + 8) * U * A).reshape(n, 1, 1, C)


def gdc_tail_layer(desc, params, x, dtype=torch.float64, eps=L2_EPS):
    """gdc_tail_kernel<KSPLIT> / gdc_tail_a_kernel + gdc_tail_b_kernel: a as dwfull_layer, b = a Wpw (K = 512), o = b Wd
    (K = E), y = o / sqrt(max(sum o^2, eps)) -> ([n, 1, 1, E], B).  The bound goes stage by stage, in float64:
        da = (HW + 8) u A~a
        db = da |Wpw| + 512 u (|a| |Wpw|)
        do = db |Wd| + E u (|b| |Wd|)
        B  = do / ||o|| + |y| ||do||_2 / ||o|| + (E / 2 + 4) u |y|
    (the error of o carried through the division, through the norm -- | ||o + d|| - ||o|| | <= ||d|| --, and the
    normalisation's own rounding as l2norm_layer).  With every o zero and do zero (a zero dense kernel) B is 0: the clamp
    makes the row exactly 0.  B is of the float64 run whatever `dtype` computes the chain in."""
    if desc['kind'] != 'gdctail':
        raise NotUnderstood('gdc_tail_layer on %r' % desc['kind'])
    E = desc['cout']
    HW = desc['k'][0] * desc['k'][1]

    def chain(dt):
        a, A = _depthwise_full(desc, params, x, dt)
        wpw = _p(params, desc['w_pw'], a).reshape(-1, E)
        wd = _p(params, desc['w_dense'], a).reshape(E, E)
        if wpw.shape[0] != a.shape[1]:
            raise NotUnderstood('1x1 kernel %s on %d channels' % (tuple(wpw.shape), a.shape[1]))
        b = a @ wpw
        o = b @ wd
        nrm = torch.sqrt((o * o).sum(1, keepdim=True).clamp_min(eps))
        return a, A, wpw, wd, b, o, nrm, o / nrm

    a, A, wpw, wd, b, o, nrm, y = chain(torch.float64)
    da = (HW + 8) * U * A
    db = da @ wpw.abs() + a.shape[1] * U * (a.abs() @ wpw.abs())
    do = db @ wd.abs() + E * U * (b.abs() @ wd.abs())
    B = do / nrm + y.abs() * do.norm(dim=1, keepdim=True) / nrm + (E / 2 + 4) * U * y.abs()
    if dtype != torch.float64:
        y = chain(dtype)[-1]
    n = y.shape[0]
    return y.reshape(n, 1, 1, E), B.reshape(n, 1, 1, E)


def l2norm_layer(desc, x, dtype=torch.float64, eps=L2_EPS):
    """l2norm_kernel: y = x / sqrt(max(sum x^2, eps)) over the D channels of a [n, 1, 1, D] row -> (y, B = (D / 2 + 4) u |ref|):
    the sum's error enters the root by half, + the root, the reciprocal and the product."""
    _whole(desc['x'], 'x')
    if x.shape[1:3] != (1, 1) or x.shape[3] != desc['cout']:
        raise NotUnderstood('l2norm over %s' % (tuple(x.shape),))
    D = x.shape[3]
    x64 = x.to(torch.float64)
    ref = x64 / torch.sqrt((x64 * x64).sum(3, keepdim=True).clamp_min(eps))
    B = (D / 2 + 4) * U * ref.abs()
    if dtype == torch.float64:
        return ref, B
    xt = x.to(dtype)
    return xt / torch.sqrt((xt * xt).sum(3, keepdim=True).clamp_min(eps)), B


def lrn_layer(desc, x, dtype=torch.float64):
    """lrn_kernel: y = x / (bias + alpha sum_{|j - c| <= r, 0 <= j < C} x_j^2) ^ beta with the constants of the describe line
    (float32 values) -> (y, B = (P + 12) u |ref|): the up-to-11-term sum, the fma, the division and beta times the base's
    error make the 12, P = POWF_ULP is the device powf's."""
    _whole(desc['x'], 'x')
    if desc.get('lrn') is None:
        raise NotUnderstood('no lrn constants on %r' % desc['name'])
    r = desc['lrn'][0]
    bias, alpha, beta = (float(torch.tensor(v, dtype=torch.float32)) for v in desc['lrn'][1:])      # the float32 values the kernel gets
    if 2 * r + 1 > 11:
        raise NotUnderstood('lrn radius %d: the bound counts at most 11 terms' % r)
    C = x.shape[3]

    def run(dt):
        xt = x.to(dt)
        sq = torch.nn.functional.pad(xt * xt, (r, r))
        s = torch.zeros_like(xt)
        for j in range(2 * r + 1):
            s = s + sq[..., j:j + C]
        base = torch.tensor(bias, dtype=dt, device=x.device) + torch.tensor(alpha, dtype=dt, device=x.device) * s
        return xt / torch.pow(base, torch.tensor(beta, dtype=dt, device=x.device))

    ref = run(torch.float64)
    B = (POWF_ULP + 12) * U * ref.abs()
    return (ref if dtype == torch.float64 else run(dtype)), B


# ----------------------------------------------------------------------------------------------- gates
def worst(got, ref, denom):
    """max |got - ref| / denom and where: (ratio, (image, row, column, channel)).  Elements whose bound is 0 must be exact."""
    err = (got.to(torch.float64) - ref.to(torch.float64)).abs()
    ratio = torch.where(denom > 0, err / denom.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))


def rel_error(got, ref, A):
    """max over the elements with A > 0 of |got - ref| / A: the figure the tight gate compares between kernel and yardstick."""
    err = (got.to(torch.float64) - ref.to(torch.float64)).abs()
    ok = A > 0
    return float((err[ok] / A[ok]).max()) if bool(ok.any()) else 0.0


TIGHT_FACTOR = 8.0


def tight_limit(y32, ref, A):
    """8 * max(the float32 yardstick's own error on this input, 2 u), relative to A."""
    return TIGHT_FACTOR * max(rel_error(y32, ref, A), 2 * U)


def rms_error(got, ref, A):
    """rms over the elements with A > 0 of (got - ref) / A."""
    ok = A > 0
    if not bool(ok.any()):
        return 0.0
    e = (got.to(torch.float64) - ref.to(torch.float64))[ok] / A[ok]
    return float((e * e).mean().sqrt())


def rms_limit(y32, ref, A):
    """RMS_MARGIN x the float32 yardstick's rms on this input, relative to A (no floor: a yardstick at 0 asks for 0)."""
    return RMS_MARGIN * rms_error(y32, ref, A)


def gate_in_B(got, y32, ref, B):
    """The tight gate in units of B, for the layers whose B is not a multiple of one magnitude:
    (max |got - ref| / B, 8 max(max |y32 - ref| / B, max 2 u |ref| / B), where the kernel's worst sits)."""
    r, at = worst(got, ref, B)
    ry, _ = worst(y32, ref, B)
    ok = B > 0
    floor = float((2 * U * ref.abs().to(torch.float64)[ok] / B[ok]).max()) if bool(ok.any()) else 0.0
    return r, TIGHT_FACTOR * max(ry, floor), at
