"""Test helper: a textbook belief-propagation decoder of a (174, 91) code, to measure the contract's decoder against -- NOT a restatement of it.
Flooding sum-product in float64 on log-likelihood ratios, the check update by numpy.tanh / numpy.arctanh with the product clipped to
+-(1 - 1e-15); it stops on a zero syndrome or after `max_iter` iterations and has no early stop.  Of tests/ldpc_ref.py it takes the Code tables
(which bit sits at which edge) and nothing else: no Pade tanh, no piecewise atanh, no float32, another sign convention, another way of summing."""
import numpy as np

N, K, M, ROWMAX = 174, 91, 83, 7
CLIP = 1.0 - 1e-15


def decode(code, llr, max_iter=30):
    """llr [q, 174], positive for a 1 (the repository's convention) -> (cw uint8[q, 174] the hard decisions at the exit, ok bool[q]: the syndrome
    is zero, iters int[q]).  Internally lam = log P(0) / P(1) = -llr, the textbook's sign."""
    lam = -np.asarray(llr, np.float64).reshape(-1, N)
    Q = len(lam)
    present = np.asarray(code.present, bool)                           # [83, 7]
    bit = np.where(present, code.rowbit, 0)                            # [83, 7]
    inc = np.zeros((M * ROWMAX, N))                                    # edge -> bit incidence: the bit sums are one matrix product
    inc[np.nonzero(present.ravel())[0], bit.ravel()[present.ravel()]] = 1.0
    c2b = np.zeros((Q, M, ROWMAX))                                     # check -> bit messages, 0 at absent edges
    cw, ok, iters = np.zeros((Q, N), np.uint8), np.zeros(Q, bool), np.zeros(Q, int)
    live = np.arange(Q)
    for it in range(max_iter + 1):
        post = lam[live] + c2b[live].reshape(len(live), -1) @ inc      # a-posteriori ratio of every bit
        hard = post < 0
        synd = (hard[:, bit] & present).sum(axis=2) & 1
        good = ~synd.any(axis=1)
        done = good | (it == max_iter)
        cw[live[done]], ok[live[done]], iters[live[done]] = hard[done], good[done], it
        live, post = live[~done], post[~done]
        if not live.size:
            break
        b2c = post[:, bit] - c2b[live]                                 # extrinsic: everything the bit knows except what this check told it
        th = np.where(present, np.tanh(0.5 * b2c), 1.0)
        new = np.zeros_like(th)
        for e in range(ROWMAX):
            others = np.prod(np.delete(th, e, axis=2), axis=2)
            new[:, :, e] = 2.0 * np.arctanh(np.clip(others, -CLIP, CLIP))
        c2b[live] = np.where(present, new, 0.0)
    return cw, ok, iters
