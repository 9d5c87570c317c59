"""The reciprocal-space contracts of include/pdbeda.h restated in plain numpy (pdbeda_map_fft, pdbeda_spectrum_inverse, pdbeda_spectrum_scale,
pdbeda_spectrum_shells, pdbeda_spectrum_values): numpy.fft in fp64 for the transforms, and the frequency numbers, s^2 in the contract's
operation order (numpy's element-wise fp64 is unfused), the table rule and the shell rule for the rest.  Grids are [s][r][c]; a metric is
{m00, m11, m22, m01, m02, m12}.  Nothing here reads the product's code."""
import numpy as np

EPS = 2.0 ** -53


def forward(grid):
    """rfftn of a float32 grid in fp64: complex128 [ns][nr][nc // 2 + 1]."""
    return np.fft.rfftn(np.asarray(grid, dtype=np.float64))


def full(grid):
    """fftn: complex128 [ns][nr][nc]."""
    return np.fft.fftn(np.asarray(grid, dtype=np.float64))


def inverse(spec, shape):
    """irfftn onto ``shape`` = (ns, nr, nc), rounded once to float32."""
    return np.fft.irfftn(spec, s=shape, axes=(0, 1, 2)).astype(np.float32)


def forward_bound(shape):
    """The relative L2 bound of a forward transform: 16 * 2^-53 * max(1, log2 N)."""
    return 16.0 * EPS * max(1.0, float(np.log2(float(np.prod(shape)))))


def rel_l2(got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    norm = float(np.sqrt(np.sum(np.abs(want) ** 2)))
    return float(np.sqrt(np.sum(np.abs(got - want) ** 2))) / (norm if norm > 0 else 1.0)


def freq(n):
    """The frequency numbers of the indices of an axis of n: j if 2 j <= n, else j - n."""
    j = np.arange(n, dtype=np.int64)
    return np.where(2 * j <= n, j, j - n)


def s2_grid(shape, metric, half=True):
    """s^2 of every coefficient, [ns][nr][nc // 2 + 1] (or [ns][nr][nc]), in the contract's order."""
    ns, nr, nc = shape
    m = [np.float64(v) for v in metric]
    h0 = freq(nc)[: nc // 2 + 1] if half else freq(nc)
    h0, h1, h2 = h0[None, None, :], freq(nr)[None, :, None], freq(ns)[:, None, None]
    f = lambda a: a.astype(np.float64)
    d0, d1, d2 = m[0] * f(h0 * h0), m[1] * f(h1 * h1), m[2] * f(h2 * h2)
    x01, x02, x12 = m[3] * f(h0 * h1), m[4] * f(h0 * h2), m[5] * f(h1 * h2)
    return ((d0 + d1) + d2) + 2.0 * ((x01 + x02) + x12)


def gain(s2, table, s2_max, beyond):
    """g(s^2) of pdbeda_spectrum_scale."""
    table = np.asarray(table, dtype=np.float64)
    n = len(table)
    t = s2 * (np.float64(n - 1) / np.float64(s2_max))
    fl = np.floor(t)
    i = np.clip(fl.astype(np.int64), 0, n - 2)
    g = table[i] + (t - fl) * (table[i + 1] - table[i])
    g = np.where(t == n - 1, table[n - 1], g)
    g = np.where(t > n - 1, np.float64(beyond), g)
    return np.where(t >= 0.0, g, table[0])


def scaled(spec, shape, metric, table, s2_max, beyond=0.0):
    """pdbeda_spectrum_scale of a half spectrum: both components times the real g."""
    g = gain(s2_grid(shape, metric), table, s2_max, beyond)
    return spec.real * g + 1j * (spec.imag * g)


def shell_of(s2, edges):
    """The shell of every s^2 (edges[j] <= s2 < edges[j + 1]); -1 outside."""
    edges = np.asarray(edges, dtype=np.float64)
    j = np.searchsorted(edges, s2, side="right") - 1
    return np.where((j >= 0) & (j < len(edges) - 1), j, -1)


def _fold(shell, weight, a, b, n_shells):
    keep = shell >= 0
    sh, w = shell[keep], weight[keep]
    A = a[keep]
    B = b[keep] if b is not None else None
    count = np.bincount(sh, weights=w, minlength=n_shells).astype(np.int64)
    sums = np.zeros((n_shells, 4))
    sums[:, 0] = np.bincount(sh, weights=w * (A.real * A.real + A.imag * A.imag), minlength=n_shells)
    if B is not None:
        sums[:, 1] = np.bincount(sh, weights=w * (B.real * B.real + B.imag * B.imag), minlength=n_shells)
        sums[:, 2] = np.bincount(sh, weights=w * (A.real * B.real + A.imag * B.imag), minlength=n_shells)
        sums[:, 3] = np.bincount(sh, weights=w * (A.imag * B.real - A.real * B.imag), minlength=n_shells)
    return count, sums


def shells(spec_a, spec_b, shape, metric, edges):
    """(count, sums [n][4]) of pdbeda_spectrum_shells from HALF spectra with the weights 1 / 2."""
    ns, nr, nc = shape
    s2 = s2_grid(shape, metric)
    col = np.arange(nc // 2 + 1)
    w = np.where((col == 0) | (2 * col == nc), 1.0, 2.0)
    weight = np.broadcast_to(w[None, None, :], s2.shape)
    return _fold(shell_of(s2, edges).ravel(), weight.ravel(), spec_a.ravel(), None if spec_b is None else spec_b.ravel(), len(edges) - 1)


def shells_full(full_a, full_b, shape, metric, edges):
    """The same sums from FULL spectra, every coefficient once."""
    s2 = s2_grid(shape, metric, half=False)
    return _fold(shell_of(s2, edges).ravel(), np.ones(s2.size), full_a.ravel(), None if full_b is None else full_b.ravel(), len(edges) - 1)


def edge_clearance(shape, metric, edges):
    """The smallest relative distance of any s^2 (half spectrum) to any edge."""
    s2 = s2_grid(shape, metric).ravel()
    return min(float(np.min(np.abs(s2 - e))) / float(e) for e in np.asarray(edges, dtype=np.float64))


def values(full_spec, idx):
    """Coefficients of the FULL spectrum [ns][nr][nc] at integer (k0, k1, k2) rows, each reduced modulo its axis."""
    ns, nr, nc = full_spec.shape
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    return full_spec[np.mod(idx[:, 2], ns), np.mod(idx[:, 1], nr), np.mod(idx[:, 0], nc)]


def structure_factors(header, grid, hkl):
    """F(h) = V / N sum rho exp(+2 pi i h.x) of a whole-cell map by the plain sum over its voxels; x = (index + crsStart) / interval per axis."""
    nc, nr, ns = [int(v) for v in header.ncrs]
    g = np.asarray(grid, dtype=np.float64)
    volume = float(header.unitVolume) * float(np.prod([float(v) for v in header.xyzInterval]))
    out = []
    for h in np.asarray(hkl, dtype=np.int64).reshape(-1, 3):
        k = [int(h[header.map2crs[a]]) for a in range(3)]      # the Miller index along each crs axis
        ph = [np.exp(2j * np.pi * k[a] * ((np.arange(n) + int(header.crsStart[a])) / float(header.crsInterval[a]))) for a, n in enumerate((nc, nr, ns))]
        out.append(volume / g.size * np.einsum("srk,s,r,k->", g, ph[2], ph[1], ph[0]))
    return np.array(out)


def shell_table(count, sums):
    """fsc, scale (self ~ k other) per shell from the sums; NaN where a denominator is 0."""
    saa, sbb, re = sums[:, 0], sums[:, 1], sums[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.sqrt(saa * sbb)
        return np.where(den > 0, re / den, np.nan), np.where(sbb > 0, re / sbb, np.nan)


def crossing(s, fsc, threshold):
    """The first downward crossing of ``threshold``, linearly interpolated in s; None if there is none."""
    for j in range(len(fsc) - 1):
        a, b = fsc[j], fsc[j + 1]
        if np.isfinite(a) and np.isfinite(b) and a >= threshold > b:
            return float(s[j] + (a - threshold) / (a - b) * (s[j + 1] - s[j]))
    return None
