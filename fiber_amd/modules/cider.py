"""CIDEr-D on the host (Vedantam et al., arXiv:1411.5726), the reward of CIDEr-optimised caption training: the project's restatement of
the reference's `CiderD(n=4, sigma=6.0, df=...).compute_score(gts, res)` (coarse_grained/fiber/modules/cider/ciderD/ciderD.py,
ciderD_scorer.py), written from the formulas.

A sentence is its whitespace-split words; its vector for n = 1..4 holds count * idf per n-gram, idf = ref_len - log(max(1, df)).  A hypothesis h
scores against a reference r, per n, the clipped cosine  sum_g min(h_g, r_g) r_g / (|h| |r|)  (the division only when both norms are non-zero)
times the Gaussian length penalty exp(-(len h - len r)^2 / (2 sigma^2)); the entry's score is the mean over n, the mean over its references,
times 10.  The lengths are counted as the reference counts them: the sum of the BIGRAM counts (its `n == 1` tests a zero-based index), one less
than the word count.

df="corpus": document frequencies come from the references of the call, one document per result entry, ref_len = log(number of entries).
df=<path>: a pickle {"ref_len": count, "document_frequency": {n-gram tuple: count}} read with encoding="latin1"; ref_len = log(float(count))."""
import math
import pickle

import numpy as np


def ngram_counts(sentence, n=4):
    """{n-gram tuple: count} for the 1..n-grams of a whitespace-split sentence, in order of first appearance per length."""
    words = sentence.split()
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


class CiderD:
    def __init__(self, n=4, sigma=6.0, df="corpus"):
        self.n, self.sigma, self.df_mode = n, sigma, df
        self.ref_len, self.document_frequency = None, None
        if df != "corpus":
            with open(df, "rb") as f:
                table = pickle.load(f, encoding="latin1")
            self.ref_len = math.log(float(table["ref_len"]))
            self.document_frequency = table["document_frequency"]

    def _vector(self, counts, doc_freq, ref_len):
        """(per-n {n-gram: tf idf}, per-n norm, length) of one sentence's counts"""
        vec = [dict() for _ in range(self.n)]
        sq = [0.0] * self.n
        length = 0
        for g, tf in counts.items():
            k = len(g) - 1
            w = float(tf) * (ref_len - math.log(max(1.0, doc_freq.get(g, 0.0))))
            vec[k][g] = w
            sq[k] += w * w
            if k == 1:                                     # the reference's length: bigram counts
                length += tf
        return vec, [math.sqrt(s) for s in sq], length

    def _similarity(self, hyp, ref):
        (hv, hn, hl), (rv, rn, rl) = hyp, ref
        penalty = math.exp(-float(hl - rl) ** 2 / (2.0 * self.sigma ** 2))
        out = np.zeros(self.n)
        for k in range(self.n):
            dot = 0.0
            for g, w in hv[k].items():
                r = rv[k].get(g, 0.0)
                dot += min(w, r) * r
            if hn[k] != 0 and rn[k] != 0:
                dot /= hn[k] * rn[k]
            out[k] = dot * penalty
        return out

    def compute_score(self, gts, res):
        """gts: {image_id: [reference sentence, ...]}; res: [{"image_id": id, "caption": [hypothesis]}, ...].
        Returns (mean score, np.ndarray of the per-entry scores, in the order of `res`)."""
        hyps, refs = [], []
        for entry in res:
            hypo, ref = entry["caption"], gts[entry["image_id"]]
            assert isinstance(hypo, list) and len(hypo) == 1 and isinstance(ref, list) and len(ref) > 0
            hyps.append(ngram_counts(hypo[0], self.n))
            refs.append([ngram_counts(r, self.n) for r in ref])
        if self.df_mode == "corpus":
            doc_freq = {}
            for entry_refs in refs:
                for g in set(g for r in entry_refs for g in r):
                    doc_freq[g] = doc_freq.get(g, 0.0) + 1.0
            ref_len = math.log(float(len(refs))) if refs else 0.0
        else:
            doc_freq, ref_len = self.document_frequency, self.ref_len
        scores = []
        for h, entry_refs in zip(hyps, refs):
            hv = self._vector(h, doc_freq, ref_len)
            total = np.zeros(self.n)
            for r in entry_refs:
                total += self._similarity(hv, self._vector(r, doc_freq, ref_len))
            scores.append(float(np.mean(total)) / len(entry_refs) * 10.0)
        scores = np.array(scores)
        return float(np.mean(scores)) if len(scores) else 0.0, scores

    def method(self):
        return "CIDEr-D"
