#!/usr/bin/env python3
"""Bit-for-bit fingerprint of the crossbar kernels (csrc/xbar_fwd.hip,
csrc/xbar_serial.hip, csrc/xbar_cells.hip), for comparing two builds.

The noise paths of these kernels are tested statistically, so a refactor that
moved a Philox counter or the order of a multiply would pass the suite. This
tool calls the C++ entry points with fixed inputs and seeds and prints one
JSON line per case:

  sha256   of the output bytes
  tele2-4  max clean y, saturation count, max |v| as exact fp32 (hex); these
           do not depend on the order of the blocks
  tele0-1  the float-atomic sums, as floats (their order is not fixed)

Cases: the five forward variants (tiled with and without bias, differential,
bit-serial J in {1, 2, 4}, bit-sliced and programmed T in {1, 2, 4} at
cell_bits 1 and 2) and xbar_program_cells; bf16, fp16, fp32; sigma mode 0
with ADC, 1 and 2 with ADC on and off; telemetry on and off; xbar_rows 32 and
128; the small shapes of tests/test_xbar_gpu.py (ragged M and K tiles,
C % 8 != 0 with tap-straddling spans, a padded weight pitch, a short last
block, several blocks).

  python tools/xbar_digest.py [--repo TREE] > a.jsonl
  python tools/xbar_digest.py --compare a.jsonl b.jsonl

--repo names the tree to import noisynet_amd from (default: this one).
--compare needs no GPU: sha256 and tele2-4 must be identical, tele0-1 within
the relative bound the tests use for the float-atomic sums. No digest is kept
in the repository: a toolchain update may change sqrtf or __cosf bits.
There is no CPU fallback.
"""

import argparse
import hashlib
import json
import os
import struct
import sys

TELE0_REL = 2.8e-6   # tests/test_xbar_gpu.py

# name -> (kind, x shape, w shape, stride, pad)
SHAPES = {
    "linear": ("linear", (130, 296), (80, 296), 1, 0),
    "convA": ("conv", (3, 5, 9, 9), (70, 5, 5, 5), 2, 2),
    "convB": ("conv", (3, 32, 6, 6), (20, 32, 3, 3), 1, 1),
}
ROWS = (32, 128)
# (sigma_mode, adc_bits)
MODES = ((0, 4), (1, 4), (1, 0), (2, 4), (2, 0))
IN_BITS = 4
DAC_BITS = {1: 4, 2: 2, 4: 1}           # J -> dac_bits
CELLS = [(t * e, e) for e in (1, 2) for t in (1, 2, 4)]   # (w_bits, cell_bits)
ADC_MAX = 3.0
FACTOR = 0.5


def f32_hex(v):
    return struct.pack('>f', v).hex()


def compare(a_path, b_path):
    def load(path):
        with open(path) as fh:
            return {r['case']: r for r in map(json.loads, fh) if 'case' in r}
    a, b = load(a_path), load(b_path)
    bad = sorted(set(a) ^ set(b))
    worst = 0.0
    for case in sorted(set(a) & set(b)):
        ra, rb = a[case], b[case]
        if any(ra[k] != rb[k] for k in ('sha256', 'tele2', 'tele3', 'tele4')):
            bad.append(case)
            continue
        for k in ('tele0', 'tele1'):
            if ra[k] is None or rb[k] is None:
                if ra[k] != rb[k]:
                    bad.append(case)
                continue
            rel = abs(ra[k] - rb[k]) / max(abs(ra[k]), abs(rb[k]), 1e-30)
            worst = max(worst, rel)
            if rel > TELE0_REL:
                bad.append(case)
    for case in bad:
        print('DIFFERENT', case)
    print('%d cases, %d differences (largest relative difference of the '
          'float-atomic sums %.3g, bound %.3g)'
          % (len(set(a) | set(b)), len(set(bad)), worst, TELE0_REL))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repo', default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(*args.compare))

    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('xbar_digest needs a GPU: nothing computed')
    from noisynet_amd import ops
    ext = ops.ext()
    ref = ops.reference
    dev = torch.device('cuda')

    def emit(case, out, tele=None):
        raw = out.detach().contiguous().cpu().view(torch.uint8).numpy()
        t = tele.cpu().tolist() if tele is not None and tele.numel() else None
        print(json.dumps({
            'case': case,
            'sha256': hashlib.sha256(raw.tobytes()).hexdigest(),
            'tele0': t[0] if t else None, 'tele1': t[1] if t else None,
            'tele2': f32_hex(t[2]) if t else None,
            'tele3': int(t[3]) if t else None,
            'tele4': f32_hex(t[4]) if t else None}), flush=True)

    def cl(t):
        t = t.to(dev)
        return t.contiguous(memory_format=torch.channels_last) \
            if t.dim() == 4 else t

    factor = torch.tensor([FACTOR], device=dev)
    none = torch.empty(0, device=dev)
    dac = ref.xbar_dac_params(1.0 / 8, dev)
    seed = 1000
    for dname, dtype in (('bf16', torch.bfloat16), ('fp16', torch.float16),
                         ('fp32', torch.float32)):
        for sname, (kind, xs, ws, stride, pad) in SHAPES.items():
            gen = torch.Generator().manual_seed(17)
            # activations on the 4-bit grid of 1/8, weights on multiples of
            # 1/64 in [-2, 2): every grid below holds them in every dtype
            x = cl((torch.randint(0, 16, xs, generator=gen).float() / 8)
                   .to(dtype))
            wq = cl((torch.randint(-128, 128, ws, generator=gen).float() / 64)
                    .to(dtype))
            wr = cl((torch.randn(ws, generator=gen) * 0.5).to(dtype))
            bias = (torch.randn(ws[0], generator=gen)).to(dtype).to(dev)
            conv = kind == 'conv'
            geo = (stride, pad) if conv else ()

            def call(name, *a):
                return getattr(ext, name + ('_conv' if conv else '_linear'))(*a)

            chips = {}
            for wb, cb in CELLS:
                # the codes of wq on the w_bits grid over [-2, 2)
                cell = ref.xbar_cell_params(4.0 / 2 ** wb, -2.0, dev)
                seed += 1
                G = ext.xbar_program_cells(wq, wb, cb, cell, 0.1, 0.02, 0.01,
                                           seed, False)
                chips[wb, cb] = (cell, G)
                emit('program/%s/%s/w%d/e%d' % (dname, sname, wb, cb), G)
            for rows in ROWS:
                for mode, bits in MODES:
                    adc = ref.xbar_adc_params(bits, ADC_MAX, dev)
                    adcu = ref.xbar_adc_params(bits, ADC_MAX, dev,
                                               unipolar=True)
                    adc = none if adc is None else adc
                    adcu = none if adcu is None else adcu
                    for telem in (False, True):
                        tag = '%s/%s/r%d/m%d/adc%d/t%d' % (
                            dname, sname, rows, mode, bits, telem)
                        seed += 1
                        tail = (mode, factor, rows, bits)
                        for bname, b in (('bias', bias), ('nobias',
                                                          none.to(dtype))):
                            emit('tiled/%s/%s' % (bname, tag), *call(
                                'xbar_fwd', x, wq, wr, b, *geo, *tail, adc,
                                seed, telem))
                        emit('diff/' + tag, *call(
                            'xbar_diff_fwd', x, wq, wr, bias, *geo, *tail,
                            adcu, seed, telem))
                        for J, D in DAC_BITS.items():
                            emit('serial/J%d/%s' % (J, tag), *call(
                                'xbar_serial_fwd', x, wq, wr, bias, *geo,
                                *tail, adc, IN_BITS, D, dac, seed, telem))
                        for (wb, cb), (cell, G) in chips.items():
                            ctag = 'w%d/e%d/%s' % (wb, cb, tag)
                            emit('cells/' + ctag, *call(
                                'xbar_cells_fwd', x, wq, bias, *geo, *tail,
                                adcu, wb, cb, cell, seed, telem))
                            emit('prog/' + ctag, *call(
                                'xbar_prog_fwd', x, wq, G, bias, *geo, *tail,
                                adcu, wb, cb, cell, seed, telem))


if __name__ == '__main__':
    main()
