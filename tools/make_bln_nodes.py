"""Writes phaser_amd/csrc/phz_bln_nodes.h: the Gauss-Hermite rules of K_blnfit and K_blntest (phz_aebln.hip) for the node counts that PHZ_BLN_Q may take.

    python tools/make_bln_nodes.py > phaser_amd/csrc/phz_bln_nodes.h

Per rule the nodes t_i of numpy.polynomial.hermite.hermgauss and v_i = w_i exp(t_i^2): hermgauss integrates f(t) exp(-t^2) as the sum of w_i f(t_i), so the
integral of F itself over the line is about the sum of v_i F(t_i).
"""
import numpy as np

QS = (16, 24, 32, 48, 64)


def main():
    print("// Gauss-Hermite nodes t and weights v = w exp(t^2) (the integral of F over the line is about the sum of v_i F(t_i)), written by tools/make_bln_nodes.py")
    print("// from numpy.polynomial.hermite.hermgauss.  The rule is chosen by PHZ_BLN_Q.")
    print("#pragma once")
    first = True
    for q in QS:
        t, w = np.polynomial.hermite.hermgauss(q)
        v = w * np.exp(t * t)
        print("#%s PHZ_BLN_Q == %d" % ("if" if first else "elif", q))
        first = False
        print("__constant__ double BLN_T[%d] = {%s};" % (q, ", ".join("%.17g" % x for x in t)))
        print("__constant__ double BLN_V[%d] = {%s};" % (q, ", ".join("%.17g" % x for x in v)))
    print("#else")
    print("#error \"PHZ_BLN_Q must be one of %s\"" % ", ".join(str(q) for q in QS))
    print("#endif")


if __name__ == "__main__":
    main()
