"""The scores of acoustic unit discovery restated in plain Python loops over labels of any
hashable type: frame counts, max-overlap mapping, normalised mutual information, entropy rate,
boundary recall / precision / F-score, token and oracle error rates (on editdist_truth)."""

import math

import editdist_truth as et


def frame_counts(ref, hyp):
    '{hyp label: {ref label: frames}} over utterances of per-frame labels, in order of appearance.'
    counts = {}
    for r_utt, h_utt in zip(ref, hyp):
        assert len(r_utt) == len(h_utt)
        for r, h in zip(r_utt, h_utt):
            row = counts.setdefault(h, {})
            row[r] = row.get(r, 0) + 1
    return counts


def mapping(counts, ref_order):
    'hyp label -> the ref label with most frames; among equals the first in `ref_order`.'
    out = {}
    for h, row in counts.items():
        best = None
        for r in ref_order:
            if r in row and (best is None or row[r] > row[best]):
                best = r
        out[h] = best
    return out


def _entropy(probs):
    return -sum(p * math.log2(p) for p in probs if p > 0)


def nmi(counts):
    total = sum(n for row in counts.values() for n in row.values())
    if total == 0:
        return 0.
    p_x = [sum(row.values()) / total for row in counts.values()]
    cols = {}
    for row in counts.values():
        for r, n in row.items():
            cols[r] = cols.get(r, 0) + n
    p_y = [n / total for n in cols.values()]
    h_x, h_y = _entropy(p_x), _entropy(p_y)
    if h_x + h_y == 0:
        return 0.
    # H(Y | X) = - sum_xy p(x, y) log2 p(y | x)
    h_y_x = 0.
    for row in counts.values():
        n_x = sum(row.values())
        for n in row.values():
            if n > 0:
                h_y_x -= n / total * math.log2(n / n_x)
    return 200. * (h_y - h_y_x) / (h_x + h_y)


def merged(seq):
    out = []
    for x in seq:
        if not out or out[-1] != x:
            out.append(x)
    return out


def entropy_rate(seqs):
    counts = {}
    for seq in seqs:
        for x in merged(seq):
            counts[x] = counts.get(x, 0) + 1
    total = sum(counts.values())
    if total == 0:
        return 0., 1.
    h = _entropy([n / total for n in counts.values()])
    return h, 2. ** h


def boundaries(labels):
    return [t for t in range(1, len(labels)) if labels[t] != labels[t - 1]]


def boundary_scores(ref, hyp, delta=2):
    '(recall, precision, fscore) in percent, and (hits, n_ref, n_hyp).'
    hits = n_ref = n_hyp = 0
    for r_utt, h_utt in zip(ref, hyp):
        rb, hb = boundaries(r_utt), boundaries(h_utt)
        n_ref, n_hyp = n_ref + len(rb), n_hyp + len(hb)
        used = [False] * len(rb)
        for b in hb:
            best = None
            for k, r in enumerate(rb):
                if not used[k] and (best is None or abs(r - b) < abs(rb[best] - b)):
                    best = k
            if best is not None and abs(rb[best] - b) <= delta:
                hits += 1
                used[best] = True
    recall = hits / n_ref if n_ref else 0.
    precision = hits / n_hyp if n_hyp else 0.
    f = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.
    return (100. * recall, 100. * precision, 100. * f), (hits, n_ref, n_hyp)


def token_errors(refs, hyps):
    '(errors, sub, del, ins, n_ref, n_utts)'
    tot = [0, 0, 0, 0]
    for r, h in zip(refs, hyps):
        tot = [a + b for a, b in zip(tot, et.edit_ops(r, h))]
    return tuple(tot) + (sum(len(r) for r in refs), len(refs))


def oracle_errors(refs, hyp_lists):
    tot = [0, 0, 0, 0]
    for r, lst in zip(refs, hyp_lists):
        ops = [et.edit_ops(r, h) for h in lst]
        best = min(range(len(ops)), key=lambda i: (ops[i][0], i))
        tot = [a + b for a, b in zip(tot, ops[best])]
    return tuple(tot) + (sum(len(r) for r in refs), len(refs))


def evaluate_lines(ref, hyps, delta=2):
    '''The lines `beer hmm evaluate` prints for `ref` (per-frame labels per utterance) and `hyps`
    (a list of hypotheses per utterance; the first is scored), and the oracle line.'''
    first = [lst[0] for lst in hyps]
    counts = frame_counts(ref, first)
    ref_order = sorted({l for utt in ref for l in utt})
    for lst in hyps:                                     # units only later ranks use
        for utt in lst:
            for l in utt:
                counts.setdefault(l, {})
    amap = mapping(counts, ref_order)
    for h in amap:
        if amap[h] is None:
            amap[h] = ref_order[0]
    refs = [merged(r) for r in ref]
    err = token_errors(refs, [merged([amap[l] for l in h]) for h in first])
    h_rate, ppl = entropy_rate(first)
    (rec, prec, f), _ = boundary_scores(ref, first, delta)

    def pct(n):
        return '%.2f' % (100. * n / err[4] if err[4] else 0.)
    lines = [f'PER {pct(err[0])}', f'sub {pct(err[1])}', f'del {pct(err[2])}', f'ins {pct(err[3])}',
             'NMI %.2f' % nmi(frame_counts(ref, first)), 'entropy_rate %.2f' % h_rate,
             'perplexity %.2f' % ppl, 'recall %.2f' % rec, 'precision %.2f' % prec,
             'fscore %.2f' % f, f'n_units {len(counts)}']
    orc = oracle_errors(refs, [[merged([amap[l] for l in h]) for h in lst] for lst in hyps])
    return lines, 'closest_PER %.2f' % (100. * orc[0] / orc[4] if orc[4] else 0.), amap
