"""The layer-tap sweep shared by tests/test_layer_taps_gpu.py and tools/layer_taps.py: for EVERY launch of a
net, one tapped forward, the float64 reference of that launch computed on the device from the very x and res the kernel
read, and every element of every image of what it stored held to the gates:

  hard, per element      |y - ref| <= B (layer_ref.bound_factor x A~), y2 the same; exact layers bit for bit
  tight, per layer       max |y - ref| / A~ <= 8 max(max |y32 - ref| / A~, 2 u)   (f32 and Winograd forms; y32: the float32
                         yardstick on the same input -- the same sum over taps, or the Winograd order of operations)
                         the fused GDC tail, l2norm and lrn: the same in units of B (layer_ref.gate_in_B)
  split-bf16 tiers       the hard bound above against the true layer, and against the SPLIT reference S of the tier in force (the
                         float64 sum of the six / three kept products of the bf16 planes: layer_ref.conv_layer(bf_terms=t)):
                           hard   |y - S| <= (NQ K M + 8) u A~ per element (layer_ref.split_bound_factor)
                           max    max |y - S| / A~ <= 8 max(yardstick's, 2 u); the yardstick: the same sum in float32 in the
                                  kernel's order of products
                           rms    rms((y - S) / A~) <= layer_ref.RMS_MARGIN x the yardstick's rms
  untouched forward      every tapped forward's outputs equal embed's, bit for bit

Failures are collected, not raised: the caller asserts on the list, so one run names every failing layer."""
import re

import torch

import layer_ref as L

WINO = ('conv_wino_kernel', 'conv_winow_kernel', 'conv_winox_kernel')


def kernel_form(kern):
    if kern.startswith(WINO):
        return 'wino'
    if 'split-bf16' in kern:
        return 'bf16'
    return 'direct'


def family(kern):
    """The label a record is kept under: the kernel's name with its tile / operand form, as op_table() gives it, without the
    split-K factor (it moves with the batch and the device's block count)."""
    return re.sub(r',S=\d+', '', kern)


def _outs(t):
    return list(t) if isinstance(t, (list, tuple)) else [t]


def _fmt(name, kern, what, ratio, at, extra=''):
    return '%s [%s] %s: ratio %.3g at image %d, pixel (%d, %d), channel %d%s' % (name, kern, what, ratio, at[0], at[1], at[2], at[3], extra)


def sweep(model, x, label='', record=None, verbose=False, params=None, kinds=None, names=None, labels=None, ref_terms=None, details=None):
    """x: the input batch on the device (uint8 or float32, NHWC).  Returns (failures, kernel labels seen, launches checked).
    record: dict kernel label -> {'hard': (ratio, layer), 'tight': (kernel / yardstick ratio, layer)}, worst kept; a split-bf16
    label also 'split<t>_hard' (|y - S| / B), 'split<t>_max' and 'split<t>_rms' (kernel / yardstick), t the tier that ran.
    labels: only the launches whose kernel label in the untapped forward of x holds one of these texts.
    ref_terms: the tier of the split reference, where a test hands the gates another than the one in force on purpose.
    details: a list that takes (name, kernel label, describe line) of every launch checked.
    params: the reference's parameters, the model's own unless a test hands it others on purpose.
    kinds / names: only the launches of these kinds / whose name starts with one of these are tapped and compared (a head
    case: a few launches of a whole net); the untouched-forward check runs for each of them."""
    params = model.get_weights() if params is None else params
    descs = model.op_describe()
    want_out = [t.clone() for t in _outs(model.embed(x))]
    scale, bias, bgr, hflip = getattr(model, '_transform', (1.0, (0.0, 0.0, 0.0), False, False))
    # the tier in force: dif_net_set_option("bf_terms") moves it at any time, DifEmbedder.set_option keeps count
    bf_terms = model.bf_terms if model.compute != 'f32' else 0
    before = model.op_table()                  # the kernels the untapped forward ran
    fails, seen, checked = [], set(), 0

    def note(kern, key, ratio, layer):
        if record is not None:
            r = record.setdefault(family(kern), {})
            if key not in r or ratio > r[key][0]:
                r[key] = (ratio, layer)

    def gated(name, kern, got, yard, ref, B):
        """A layer that returns (ref, B): the hard bound per element and the tight gate in units of B."""
        r, lim, at = L.gate_in_B(got, yard, ref, B)
        note(kern, 'hard', r, name)
        note(kern, 'tight', r / (lim / L.TIGHT_FACTOR) if lim > 0 else (0.0 if r == 0 else float('inf')), name)
        if verbose:
            print('%s %s [%s]: |y - ref| / B %.4g, tight limit %.4g' % (label, name, kern, r, lim))
        if not r <= 1.0:
            fails.append(_fmt(name, kern, '|y - ref| / B', r, at))
        if not r <= lim:
            fails.append(_fmt(name, kern, 'tight gate: |y - ref| / B = %.3g, limit %.3g; kernel / yardstick' % (r, lim),
                              r / (lim / L.TIGHT_FACTOR) if lim > 0 else float('inf'), at))

    for i, d in enumerate(descs):
        if (kinds is not None and d['kind'] not in kinds) or (names is not None and not d['name'].startswith(tuple(names))):
            continue
        if labels is not None and not any(t in before[i][1] for t in labels):
            continue
        tap = model.tap(x, i)
        name, kern, _ = model.op_table()[i]
        if details is not None:
            details.append((name, kern, d))
        seen.add(kern)
        got_out = _outs(tap['out'])
        if len(got_out) != len(want_out) or not all(torch.equal(a, b) for a, b in zip(got_out, want_out)):
            fails.append('%s [%s]: the tapped forward\'s outputs differ from embed\'s' % (name, kern))
        kind = d['kind']
        checked += 1
        try:
            if kind == 'input':
                ref = L.input_convert(x, False, scale, bias, bgr, hflip)
                if not torch.equal(tap['y'], ref):
                    r, at = L.worst(tap['y'], ref, torch.zeros_like(ref, dtype=torch.float64))
                    fails.append(_fmt(name, kern, 'not bit-exact', r, at))
            elif kind == 'maxpool' and d['pool'] != 'max':
                ref, _, B = L.pool_layer(d, params, tap['x'])
                r, at = L.worst(L.window(d['y'], tap['y']), ref, B)
                note(kern + '[' + d['pool'] + ']', 'hard', r, name)
                if not r <= 1.0:
                    fails.append(_fmt(name, kern, '%s pool |y - ref| / B' % d['pool'], r, at))
            elif kind == 'dwfull':
                ref, B = L.dwfull_layer(d, params, tap['x'])
                r, at = L.worst(L.window(d['y'], tap['y']), ref, B)
                note(kern, 'hard', r, name)
                if not r <= 1.0:
                    fails.append(_fmt(name, kern, '|y - ref| / B', r, at))
            elif kind == 'gdctail':
                ref, B = L.gdc_tail_layer(d, params, tap['x'])
                gated(name, kern, L.window(d['y'], tap['y']), L.gdc_tail_layer(d, params, tap['x'], torch.float32)[0], ref, B)
            elif kind == 'l2norm':
                ref, B = L.l2norm_layer(d, tap['x'])
                gated(name, kern, L.window(d['y'], tap['y']), L.l2norm_layer(d, tap['x'], torch.float32)[0], ref, B)
            elif kind == 'lrn':
                ref, B = L.lrn_layer(d, tap['x'])
                gated(name, kern, L.window(d['y'], tap['y']), L.lrn_layer(d, tap['x'], torch.float32)[0], ref, B)
            elif kind == 'maxpool':
                y, y2, _ = L.pool_layer(d, params, tap['x'])
                for key, ref in (('y', y), ('y2', y2)):
                    if ref is None:
                        continue
                    got = L.window(d[key], tap[key])
                    if not torch.equal(got, ref):
                        r, at = L.worst(got, ref, torch.zeros_like(ref, dtype=torch.float64))
                        fails.append(_fmt(name, kern, key + ' not bit-exact', r, at))
            elif kind in ('upsample', 'copy'):
                L._whole(d['x'], 'x')
                ref = L.upsample_layer(tap['x']) if kind == 'upsample' else tap['x']
                got = L.window(d['y'], tap['y'])
                if not torch.equal(got, ref):
                    r, at = L.worst(got, ref, torch.zeros_like(ref, dtype=torch.float64))
                    fails.append(_fmt(name, kern, 'not bit-exact', r, at))
            elif kind == 'zero':
                if bool((L.window(d['y'], tap['y']) != 0).any()):
                    fails.append('%s [%s]: not zero' % (name, kern))
            elif kind == 'dwconv':
                ref, A = L.dwconv_layer(d, params, tap['x'])
                K = d['k'][0] * d['k'][1]
                r, at = L.worst(L.window(d['y'], tap['y']), ref, (K + 8) * L.U * A)
                note(kern, 'hard', r, name)
                if not r <= 1.0:
                    fails.append(_fmt(name, kern, '|y - ref| / B', r, at))
            elif kind == 'conv':
                form = kernel_form(kern)
                ry, ry2, A, A2 = L.conv_layer(d, params, tap['x'], tap.get('res'), torch.float64, form)
                f = L.bound_factor(d, form, bf_terms)
                y32 = y32_2 = None
                if form != 'bf16':
                    y32, y32_2, _, _ = L.conv_layer(d, params, tap['x'], tap.get('res'), torch.float32, form)
                split = {}
                if form == 'bf16':
                    terms = ref_terms or bf_terms
                    if terms not in L.BF_KEPT:
                        raise L.NotUnderstood('a split-bf16 kernel with %r terms in force' % (terms,))
                    sy, sy2, _, _ = L.conv_layer(d, params, tap['x'], tap.get('res'), torch.float64, form, terms)
                    yy, yy2, _, _ = L.conv_layer(d, params, tap['x'], tap.get('res'), torch.float32, form, terms)
                    split, fs, tag = {'y': (sy, yy), 'y2': (sy2, yy2)}, L.split_bound_factor(d, terms), 'split%d_' % terms
                for key, ref, mag, yard in (('y', ry, A, y32), ('y2', ry2, A2, y32_2)):
                    if ref is None:
                        continue
                    got = L.window(d[key], tap[key])
                    if key in split:
                        S, Y = (L.stored(d, key, t) for t in split[key])
                        m = L.stored(d, key, mag)
                        if got.shape != S.shape:
                            raise L.NotUnderstood('%s stored as %s, reference %s' % (key, tuple(got.shape), tuple(S.shape)))
                        r, at = L.worst(got, S, fs * m)
                        rel, lim, yrel = L.rel_error(got, S, m), L.tight_limit(Y, S, m), L.rel_error(Y, S, m)
                        rms, yrms = L.rms_error(got, S, m), L.rms_error(Y, S, m)
                        ratio = rms / yrms if yrms > 0 else (0.0 if rms == 0 else float('inf'))
                        if ref_terms is None:
                            note(kern, tag + 'hard', r, name)
                            note(kern, tag + 'max', rel / max(yrel, 2 * L.U), name)
                            note(kern, tag + 'rms', ratio, name)
                        if verbose:
                            print('%s %s [%s] %s, %d terms: |y - S| / B %.4g, max %.3g (yardstick %.3g), rms %.3g (yardstick %.3g, x %.3g)'
                                  % (label, name, kern, key, terms, r, rel, yrel, rms, yrms, ratio))
                        if not r <= 1.0:
                            fails.append(_fmt(name, kern, 'split reference, %d terms: |%s - S| / B' % (terms, key), r, at))
                        if not rel <= lim:
                            fails.append(_fmt(name, kern, 'max gate on %s against the split reference, %d terms: |y - S| / A~ = %.3g, limit %.3g; kernel / yardstick'
                                              % (key, terms, rel, lim), rel / (lim / L.TIGHT_FACTOR), at))
                        if not ratio <= L.RMS_MARGIN:
                            fails.append(_fmt(name, kern, 'rms gate on %s against the split reference, %d terms: rms (y - S) / A~ = %.3g, yardstick %.3g, margin %.3g; kernel / yardstick'
                                              % (key, terms, rms, yrms, L.RMS_MARGIN), ratio, at))
                    ref, mag = L.stored(d, key, ref), L.stored(d, key, mag)
                    if got.shape != ref.shape:
                        raise L.NotUnderstood('%s stored as %s, reference %s' % (key, tuple(got.shape), tuple(ref.shape)))
                    r, at = L.worst(got, ref, f * mag)
                    note(kern, 'hard', r, name)
                    if verbose:
                        print('%s %s [%s] %s: |y - ref| / B %.4f' % (label, name, kern, key, r))
                    if not r <= 1.0:
                        fails.append(_fmt(name, kern, '|%s - ref| / B' % key, r, at, ' (K = %d, form %s)' % (d['k'][0] * d['k'][1] * d['cin_true'], form)))
                    if yard is not None:
                        yard = L.stored(d, key, yard)
                        rel, lim = L.rel_error(got, ref, mag), L.tight_limit(yard, ref, mag)
                        note(kern, 'tight', rel / (lim / L.TIGHT_FACTOR), name)
                        if not rel <= lim:
                            _, at = L.worst(got, ref, mag)
                            fails.append(_fmt(name, kern, 'tight gate on %s: |y - ref| / A~ = %.3g, limit %.3g; kernel / yardstick' % (key, rel, lim),
                                              rel / (lim / L.TIGHT_FACTOR), at))
            else:
                raise L.NotUnderstood('launch kind %r' % kind)
        except L.NotUnderstood as e:
            fails.append('%s [%s]: the reference does not understand this launch: %s' % (name, kern, e))
    return fails, seen, checked
