"""numpy statement of the two packings evc_fci_trdm_rows_packed writes (include/evcont_hip.h), shared by
tests/test_fci_pack_host.py (which checks it against synthetic.pack_rows and evaluator.sym8_column_images) and the GPU
tests of the packed row call."""
import numpy as np


def pack_cols(layout, n):
    n2, ms = n * n, n * (n + 1) // 2
    return ms * (ms + 1) // 2 if layout == "sym8" else n2 * (n2 + 1) // 2


def pack2_row(dm2):
    """Column R(R+1)/2 + C, R = pN+q >= C = rN+s, holds dm2[p,q,r,s]."""
    n = dm2.shape[0]
    r, c = np.tril_indices(n * n)
    return np.ascontiguousarray(dm2.reshape(n * n, n * n)[r, c])


def sym8_indices(n):
    """(i, j, k, l) of every column u(u+1)/2 + v, u = i(i+1)/2+j (i >= j), v = k(k+1)/2+l (k >= l), u >= v."""
    iu, ju = np.tril_indices(n)
    U, V = np.tril_indices(len(iu))
    return iu[U], ju[U], iu[V], ju[V]


def sym8_row(dm2, dtype=np.float64):
    """0.125 * (((((((d0+d1)+d2)+d3)+d4)+d5)+d6)+d7) over the eight images, in the order of the header."""
    i, j, k, l = sym8_indices(dm2.shape[0])
    d = np.asarray(dm2, dtype=dtype)
    acc = d[i, j, k, l].copy()
    for im in ((j, i, k, l), (i, j, l, k), (j, i, l, k), (k, l, i, j), (l, k, i, j), (k, l, j, i), (l, k, j, i)):
        acc = acc + d[im]
    return acc * dtype(0.125)


def pack_row(layout, dm2, dtype=np.float64):
    return sym8_row(dm2, dtype) if layout == "sym8" else pack2_row(np.asarray(dm2, dtype=dtype))
