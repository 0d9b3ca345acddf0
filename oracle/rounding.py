"""oracle/rounding.py -- TEST INFRASTRUCTURE: the constants of the derived rounding bounds that the edge tests of the
second and third kernel assert (oracle/bwk.py, oracle/nlk.py)."""
GAMMA_U = 2.0 ** -53


def gamma(m):
    """m u / (1 - m u), u = 2^-53: the standard bound of m accumulated relative roundings (Higham, Accuracy and
    Stability of Numerical Algorithms, Lemma 3.1).  It holds for any evaluation order, and FMA contraction only
    removes roundings."""
    return m * GAMMA_U / (1.0 - m * GAMMA_U)
