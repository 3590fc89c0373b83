/* tb_state.h -- the digest of a render state, one function for the host and the device.
 *
 * A render state is the two accumulation surfaces plus the frame range they hold; a state file carries them from one process to the
 * next (tb_state_save / tb_state_load, include/tracerboy_hip.h).  What proves that the bits arrived is this digest:
 *
 *   fmix64(k):  k ^= k >> 33;  k *= 0xff51afd7ed558ccd;  k ^= k >> 33;  k *= 0xc4ceb9fe1a85ec53;  k ^= k >> 33     (MurmurHash3's finalizer)
 *   digest(w[0..n)) = sum over i of fmix64((uint64(i) << 32) | w[i])   mod 2^64        (w: the data as 32-bit words)
 *
 * Every word is mixed together with its index, so two words that trade places change the value; the terms are ADDED, so the sum may be
 * taken in any order -- lanes, waves and workgroups of the device kernel (state_kernels.hip) reduce however the launch happens to be
 * shaped and still arrive at the value the host loop below computes.  The function sees bits, not floats: -0, denormals and NaN payloads
 * all count.  Like tb_math.h the header is plain C++ that hipcc compiles for both sides.
 */
#ifndef TB_STATE_H
#define TB_STATE_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TB_STATE_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define TB_STATE_HD inline
#endif

TB_STATE_HD uint64_t tb_state_fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

/* the term of word `w` at index `i` (the index enters with its low 32 bits) */
TB_STATE_HD uint64_t tb_state_term(uint64_t i, uint32_t w) { return tb_state_fmix64((i << 32) | (uint64_t)w); }

/* A running digest over a stream of words: arrays appended one after the other continue the index.  Bytes that do not fill a word are
 * padded with zeros. */
typedef struct TbStateDigest { uint64_t sum, index; } TbStateDigest;

TB_STATE_HD void tb_state_digest_words(TbStateDigest* d, const uint32_t* w, uint64_t n)
{
    uint64_t s = d->sum; const uint64_t i0 = d->index;
    for (uint64_t i = 0; i < n; i++) s += tb_state_term(i0 + i, w[i]);
    d->sum = s; d->index = i0 + n;
}

inline void tb_state_digest_bytes(TbStateDigest* d, const void* p, uint64_t bytes)
{
    const uint8_t* b = (const uint8_t*)p;
    if (((uintptr_t)b & 3u) == 0) tb_state_digest_words(d, (const uint32_t*)b, bytes / 4);
    else for (uint64_t i = 0; i < bytes / 4; i++) { uint32_t w; memcpy(&w, b + 4 * i, 4); tb_state_digest_words(d, &w, 1); }
    if (bytes & 3u) { uint32_t w = 0; memcpy(&w, b + (bytes & ~(uint64_t)3), (size_t)(bytes & 3u)); tb_state_digest_words(d, &w, 1); }
}

/* an array of a scene: its length in bytes (two words, low first), then its bytes */
inline void tb_state_digest_array(TbStateDigest* d, const void* p, uint64_t bytes)
{
    const uint32_t len[2] = {(uint32_t)bytes, (uint32_t)(bytes >> 32)};
    tb_state_digest_words(d, len, 2);
    if (p && bytes) tb_state_digest_bytes(d, p, bytes);
}

#endif /* TB_STATE_H */
