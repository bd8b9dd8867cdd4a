"""TEST INFRASTRUCTURE: float64 model of the scan noise, draw by draw (NumPy and math only: no import of the oracle, of ref
or of nav_gym_amd).

The draw (navmath.hpp mix64 / hash4, navsim_device.hpp noise_stream / gauss_noise, read as a specification).  All integer
arithmetic wraps: 64-bit for the stream, 32-bit per beam.
  mix64(z):        z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
  hash4(s,a,b,c):  h = mix64(s ^ 0x6E6176676D796D), then h = mix64(h ^ a), mix64(h ^ b), mix64(h ^ c)
  stream:          hash4(seed ^ key, genv, key, 0x6E6F697365)
  beam k:          a = low32(stream) ^ k * 0x9E3779B9, finalised (a ^= a >> 16, *= 0x7FEB352D, ^= a >> 15, *= 0x846CA68B, ^= a >> 16);
                   b = high32(stream) ^ a, half finalised (b ^= b >> 16, *= 0x7FEB352D, ^= b >> 15)
  u1 = fl32((a >> 8) + 1) * 2^-24 in [2^-24, 1],  a2 = fl32(b >> 8) * fl32(6.28318530718f * 2^-24): float32 values, and exact ones
                   (a 24-bit integer and its successor are float32 numbers, the power of two scales exactly)
  g = sqrt(-2 ln u1) cos a2, here in float64.  The device evaluates it in float32 (v_log_f32, a 1-ulp square root, __cosf).
A range r that the clip left at range_max stays; every other becomes r + std * g, float64 here, rounded twice in float32 on
the device.  That difference belongs to the tolerance of whoever compares, not to the model.

The key schedule, checked against kernels_step.hpp (phase 0 sets sh.step_key / sh.rescan_key, phase 4 replaces rescan_key
for a restart, scan B's pass 0 uses step_key + 1) and kernels_reset.hpp's callers of the same step_arena:
  genv = env_index_base + e;
  a first observation -- a reset-only launch, reset_obs, a reset_mask arena under NEXT_STEP, the restart scan inside a
  SAME_STEP step -- uses episode << 32, with the NEW episode's number;
  the first scan of a step uses (episode << 32) + 2 * steps, steps AFTER the step's increment;
  the crash re-scan uses that key + 1;
  a final_obs row carries its terminal row's key: the re-scan's after a crash, the first scan's after a success or a
  truncation."""
import math

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
TWO_PI_24 = np.float32(6.28318530718) * np.float32(2.0 ** -24)        # the device's constant 6.28318530718f / 16777216.0f
_U64 = np.uint64


# ---- integers ---------------------------------------------------------------------------------------------------------------------
def _u64(x):
    """uint64 array of Python ints or arrays (values taken modulo 2^64)"""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.asarray(int(x) & M64, dtype=np.uint64)


def mix64(z):
    with np.errstate(over="ignore"):
        z = _u64(z) + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def hash4(seed, a, b, c):
    h = mix64(_u64(seed) ^ _U64(0x6E6176676D796D))
    h = mix64(h ^ _u64(a))
    h = mix64(h ^ _u64(b))
    return mix64(h ^ _u64(c))


def noise_stream(seed, genv, scan_key):
    """uint64, broadcast over its arguments"""
    return hash4(_u64(seed) ^ _u64(scan_key), genv, scan_key, 0x6E6F697365)


def beam_fields(stream, beams):
    """(a >> 8, b >> 8): the two 24-bit fields of beam `beams` of `stream`, uint32, element by element (broadcast)"""
    stream = _u64(stream)
    k = np.asarray(beams, dtype=np.uint32)
    with np.errstate(over="ignore"):
        a = (stream & _U64(M32)).astype(np.uint32) ^ (k * np.uint32(0x9E3779B9))
        a ^= a >> np.uint32(16); a *= np.uint32(0x7FEB352D); a ^= a >> np.uint32(15); a *= np.uint32(0x846CA68B); a ^= a >> np.uint32(16)
        b = (stream >> _U64(32)).astype(np.uint32) ^ a
        b ^= b >> np.uint32(16); b *= np.uint32(0x7FEB352D); b ^= b >> np.uint32(15)
    return a >> np.uint32(8), b >> np.uint32(8)


def stream_for_fields(a_final, b_final, beam):
    """The 64-bit stream whose beam `beam` finalises to the 32-bit words (a_final, b_final): the finalisers run backwards
    (a xor-shift by s >= 16 undoes itself, one by 15 takes two rounds, the multipliers are odd).  Python ints."""
    inv1, inv2 = pow(0x7FEB352D, -1, 1 << 32), pow(0x846CA68B, -1, 1 << 32)
    a = a_final & M32
    a ^= a >> 16; a = a * inv2 & M32; a ^= a >> 15; a ^= a >> 30; a = a * inv1 & M32; a ^= a >> 16
    lo = a ^ (beam * 0x9E3779B9 & M32)
    b = b_final & M32
    b ^= b >> 15; b ^= b >> 30; b = b * inv1 & M32; b ^= b >> 16
    hi = b ^ (a_final & M32)
    return lo | hi << 32


# ---- floats -----------------------------------------------------------------------------------------------------------------------
def uniform_inputs(fa, fb):
    """(u1, a2) as float32 arrays from the 24-bit fields"""
    u1 = (fa.astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)
    a2 = fb.astype(np.float32) * TWO_PI_24
    return u1, a2


def gauss_from_fields(fa, fb):
    u1, a2 = uniform_inputs(fa, fb)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(a2.astype(np.float64))


def gauss_at(stream, beams):
    """float64 g of beam beams[i] of stream[i]"""
    return gauss_from_fields(*beam_fields(stream, beams))


def gauss(stream, beams):
    """float64 g of every beam of every stream: shape stream.shape + beams.shape"""
    return gauss_at(_u64(stream)[..., None], beams)


def noisy(clean, std, stream, range_max):
    """clean float32 [..., B] (clipped), std and stream [...] -> float64 [..., B]"""
    clean = np.asarray(clean, np.float32)
    g = gauss(stream, np.arange(clean.shape[-1]))
    out = clean.astype(np.float64) + np.asarray(std, np.float32).astype(np.float64)[..., None] * g
    return np.where(clean == np.float32(range_max), clean.astype(np.float64), out)


# ---- keys -------------------------------------------------------------------------------------------------------------------------
def first_obs_key(episode):
    return (int(episode) << 32) & M64


def step_key(episode, steps_now):
    """steps_now: the arena's step counter AFTER the step's increment"""
    return ((int(episode) << 32) + 2 * int(steps_now)) & M64


def rescan_key(episode, steps_now):
    return (step_key(episode, steps_now) + 1) & M64


def moments(x):
    """(mean, std, kurtosis) of a sample"""
    x = np.asarray(x, np.float64).ravel()
    m = x.mean()
    v = x.var()
    return m, math.sqrt(v), float(np.mean((x - m) ** 4) / v ** 2)


def correlation(x, y):
    x = np.asarray(x, np.float64).ravel() - np.mean(x)
    y = np.asarray(y, np.float64).ravel() - np.mean(y)
    return float(np.dot(x, y) / math.sqrt(np.dot(x, x) * np.dot(y, y)))
