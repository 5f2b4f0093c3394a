/* oracle/mlp_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference's MLP decode path (tuffy/libdvd-audio
 * src/mlp.c) used as the parity checker for the HIP path.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this; the
 * product (libdvd-audio_amd/) never does.
 *
 * Pinning: the reference ships no MLP vectors, so this oracle
 * is pinned against the reference itself compiled in the dev container
 * (oracle/_ref/libdvda_ref.so, built by oracle/Makefile) over seeded synthetic
 * streams, and against the committed fixtures in tests/golden/ that were
 * produced by that same reference build (tests/golden/make_golden.py).
 */
#ifndef MLP_ORACLE_H
#define MLP_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error bits accumulated in mlp_oracle_status(); 0 = every frame decoded the
 * way the reference decodes a well-formed stream.  Where the reference would
 * assert()/abort or read out of bounds, the oracle sets a bit instead. */
#define MLP_ORA_ERR_NO_SYNC      (1u << 0)  /* frame before any major sync           */
#define MLP_ORA_ERR_SYNC_CHANGE  (1u << 1)  /* later major sync differs: frame dropped (mlp.c:450-455) */
#define MLP_ORA_ERR_PARITY       (1u << 2)  /* mlp.c:692-697                         */
#define MLP_ORA_ERR_CRC          (1u << 3)  /* mlp.c:701-706                         */
#define MLP_ORA_ERR_EOF          (1u << 4)  /* read past frame/substream end         */
#define MLP_ORA_ERR_RESTART      (1u << 5)  /* mlp.c:834-848                         */
#define MLP_ORA_ERR_PARAMS       (1u << 6)  /* mlp.c:902,975,1009-1014,1035-1062...  */
#define MLP_ORA_ERR_HUFFMAN      (1u << 7)  /* invalid code, mlp.c:1228              */
#define MLP_ORA_ERR_FILTER       (1u << 8)  /* mlp.c:1260-1264                       */
#define MLP_ORA_ERR_ENVELOPE     (1u << 9)  /* reference would invoke UB*/

typedef struct mlp_oracle mlp_oracle;

mlp_oracle *mlp_oracle_open(unsigned nch);
void mlp_oracle_close(mlp_oracle *d);

/* appends `len` bytes to the decoder's queue and decodes every complete frame
 * (reference mlp.c:344-382).  Returns PCM frames decoded by this call. */
unsigned mlp_oracle_decode_packet(mlp_oracle *d, const uint8_t *data, size_t len);

unsigned mlp_oracle_status(const mlp_oracle *d);
size_t mlp_oracle_channel_len(const mlp_oracle *d, unsigned c);
const int32_t *mlp_oracle_channel(const mlp_oracle *d, unsigned c);
size_t mlp_oracle_queued_bytes(const mlp_oracle *d);

/* one-shot helper with the same shape as oracle/ref_driver.c:ref_mlp_decode.
 * out is planar [nch][cap].  Returns PCM frames, or -1 when cap is too small;
 * *status receives the error bits. */
long mlp_oracle_decode(const uint8_t *data, size_t len, size_t chunk,
                       unsigned nch, int32_t *out, size_t cap,
                       unsigned *status);

/* Optional statistics of a decode, for the tests that ask how far into the arithmetic a stream reaches and which
 * parameter values it carries.  The four peaks are taken in 64 bits before anything is narrowed to int32, so a value
 * of 2^31 or more in peak_sum / peak_output means the stream left the envelope although the decode
 * went through.  The decode itself is the same with or without statistics. */
typedef struct mlp_oracle_stats {
    uint64_t peak_filter_acc;   /* |sum of FIR and IIR products|, mlp.c:1285-1291                              */
    uint64_t peak_matrix_acc;   /* |sum of matrix products|, mlp.c:1342-1348                                   */
    uint64_t peak_sum;          /* |(acc >> shift) + residual| and |value - (acc >> shift)|, mlp.c:1293-1299   */
    uint64_t peak_output;       /* |matrix result| and |value * 2^output_shift|, mlp.c:1349-1355, 522 / 592    */
    int64_t value_min, value_max; /* extremes of (acc >> shift) + residual                                     */
    /* how often a parameter value was read (filters: those with taps) */
    uint32_t output_shift[8], qss[16], noise_shift[16], matrix_frac[15];
    uint32_t fir_shift[16], iir_shift[16], fir_coeff_shift[8], iir_coeff_shift[8];
    uint32_t fir_order[9], iir_order[9], state_bits[16], state_shift[16];
    uint32_t split8[9];         /* blocks filtered with FIR order k and IIR order 8 - k                         */
    uint32_t fir_min_rail, fir_max_rail, iir_min_rail, iir_max_rail, matrix_min_rail, matrix_max_rail;
    uint32_t lsbs_with_book[25];
    int32_t offset_min, offset_max;
    uint32_t state_top_bit_max; /* largest state_bits - 1 + state_shift                                         */
    uint32_t shift_plus_qss_max; /* largest filter shift + quant_step_size of a block filtered with taps       */
} mlp_oracle_stats;

/* mlp_oracle_decode that also adds the decode's statistics to *stats (may be NULL; the caller zeroes it) */
long mlp_oracle_decode_stats(const uint8_t *data, size_t len, size_t chunk,
                             unsigned nch, int32_t *out, size_t cap,
                             unsigned *status, mlp_oracle_stats *stats);

/* test hooks (bit-reader contract, tables) */
int mlp_oracle_test_read(const uint8_t *data, size_t len, const int *widths, int n, long *out);
int mlp_oracle_test_crc8(unsigned i);
int mlp_oracle_test_huff(unsigned book, unsigned peek9);

#ifdef __cplusplus
}
#endif
#endif
