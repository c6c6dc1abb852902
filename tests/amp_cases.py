"""Cases of the mixed-precision sparse conv tests (test_spconv_amp_gpu.py): float32 master weights and bias beside the 16-bit operands
of half_cases.py, whose geometry and oracle results these tests share.  Host only; every array is built once per process.

`unrepresentable(shape, dtype, seed)`: float32 standard-normal values, none of which is a value of `dtype`, with the first slots
overwritten by the values where a rounding can go wrong:
  exact ties in both directions: 1 + u and 1 + 3u, u = half a unit in the last place of 1 (2^-8 for bfloat16, 2^-11 for float16):
      the first rounds DOWN to the even 1, the second UP to the even 1 + 4u;
  float16's subnormal range: +-3 2^-24 (a float16 subnormal; a normal bfloat16 value after rounding) and 2^-25 (float16: the tie
      between 0 and the smallest subnormal, rounds to 0);
  -0.0, whose sign has to survive.
No infinity and no NaN, so that results can be compared as bit patterns."""
import functools

import numpy as np
import torch

import half_cases

TIE = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
N_SPECIAL = 6


def specials(dtype):
    u = TIE[dtype]
    return np.array([1.0 + u, 1.0 + 3.0 * u, 3.0 * 2.0 ** -24, -3.0 * 2.0 ** -24, 2.0 ** -25, -0.0], np.float32)


@functools.lru_cache(maxsize=None)
def unrepresentable(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32)
    back = torch.from_numpy(a).to(dtype).float().numpy()
    same = back == a                       # (probability 2^-13 / 2^-16 per element: nudged by one fp32 unit in the last place)
    a[same] = np.nextafter(a[same], np.float32(4.0))
    flat = a.reshape(-1)
    assert flat.size > 2 * N_SPECIAL
    flat[:N_SPECIAL] = specials(dtype)
    body = flat[N_SPECIAL:]
    assert (torch.from_numpy(body.copy()).to(dtype).float().numpy() != body).all() and np.isfinite(flat).all()
    a.setflags(write=False)
    return a


def weights(cin, cout, dtype):
    """[3, 3, 3, cin, cout] float32 conv weights that are not values of `dtype` (specials in the first slots)."""
    return unrepresentable((3, 3, 3, cin, cout), dtype, 7000 + 100 * cin + cout)


def bias(cout, dtype):
    """[cout] float32 bias, no element a value of `dtype`, of the size of the conv's results (no specials: c_out may be 7)."""
    rng = np.random.default_rng(9000 + cout)
    b = (rng.standard_normal(cout) * 3.0).astype(np.float32)
    back = torch.from_numpy(b).to(dtype).float().numpy()
    b[back == b] = np.nextafter(b[back == b], np.float32(100.0))
    assert (torch.from_numpy(b).to(dtype).float().numpy() != b).all()
    return b


def tables(case):
    """tab_out [K, n_dst] of the case's rulebook from the oracle's pair lists: the source row of destination row o at offset k, or -1."""
    pairs, num = case["pairs"], case["num"]
    tab = np.full((pairs.shape[0], case["n_dst"]), -1, np.int32)
    for k in range(pairs.shape[0]):
        tab[k, pairs[k, 1, :num[k]]] = pairs[k, 0, :num[k]]
    return tab


WGRAD_CHANNELS = [(32, 64), (24, 40), (160, 144)]   # aligned fetch; element-wise fetch; more than one 128-wide block of dW
BIAS_CHANNELS = [(32, 64), (5, 16), (160, 144)]
CHAIN_ROWS, CHAIN_BATCH, CHAIN_SHAPE = half_cases.ROWS, half_cases.BATCH, list(half_cases.SHAPE)
