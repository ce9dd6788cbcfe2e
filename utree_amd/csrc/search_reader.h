/* search_reader.h -- stage 1 of the host pipeline (search.c), one step per slot: read the next chunk of the input(s) and frame it.  Plain host
 * code: no device, no threads; whose memory a slot's arrays are is the caller's business. */
#ifndef UTREE_SEARCH_READER_H
#define UTREE_SEARCH_READER_H
#include <sys/types.h>
#include <zlib.h>
#include "utree_internal.h"

enum { PAIRS_NONE = 0, PAIRS_TWO_FILES, PAIRS_INTERLEAVED };

/* one input file: plain (a team of pread) or, with an opt-in format, through zlib (plain and gzip alike) */
typedef struct { int fd; gzFile gz; off_t pos; int eof; } input_t;

/* the framed arrays of one input in one slot: max_reads entries each, and `chunk` + 64 bytes at buf (interleaved mates: no buf, their spans
 * are in the reads'); rel_off is the gpu stage's */
typedef struct {
    uint8_t *buf;
    uint64_t *seq_off, *name_off, *rel_off;
    uint32_t *seq_len, *name_len;
} frames_t;

/* what a slot did not commit: framed records [from, nr) and the bytes behind them */
typedef struct {
    const uint8_t *buf; const uint64_t *name_off, *seq_off; const uint32_t *seq_len;
    size_t from, nr, used, have;
} carry_t;

typedef struct {
    input_t in[2];                              /* input; [1]: the mates file of a paired search             */
    int input_format;                           /* UTREE_INPUT_*; AUTO is resolved at the first bytes        */
    int paired;                                 /* PAIRS_*                                                   */
    size_t chunk, max_reads;                    /* bytes, and reads or pairs, a slot holds per input         */
    const char *reads_path, *mates_path;        /* as the UTREE_E_PAIRS text names them                      */
    char *msg_pairs; size_t msg_cap;            /* the caller's, for that text                               */
    size_t carry; const uint8_t *carry_src;     /* single reads: bytes of an incomplete read carried into the next chunk */
    carry_t cy[2];                              /* pairs: ... of each file                                   */
    uint64_t recs[2], pairs;                    /* records of each file, pairs, committed by the slots before */
} reader_t;

/* a filled slot: nr reads (pairs) framed in `used` of the reads buffer's `have` bytes; frame_rc UTREE_OK, or UTREE_E_FASTA (ferr) /
 * UTREE_E_PAIRS (msg_pairs) behind the nr good ones; last: the input ends with this slot */
typedef struct {
    size_t nr, have, used;
    int frame_rc, last;
    utree_fasta_error ferr;
    double t_read, t_frame;
} reader_outcome;

/* Fill one slot.  Nonzero: an error that ends the search at once (UTREE_E_IO, or a framing code other than UTREE_E_FASTA). */
int reader_step(reader_t *R, frames_t *f, reader_outcome *o);
int reader_pairs_step(reader_t *R, frames_t *f1, frames_t *f2, reader_outcome *o);

#endif
