/* search_reader.c -- stage 1 of the host pipeline (search.c): read the next chunk of the input into a slot's buffer and frame the reads
 * (fasta.c; the reference does this under `omp critical`, itree.c:867-874 -- its scaling limit).  A paired search frames both inputs and commits
 * the pairs both buffers hold.  One call fills one slot; the caller's thread owns the slots and their order. */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include "search_reader.h"
#include "search_dev.h"

#define READ_THREADS 4

/* more of `in` behind buf[0 .. *have), up to `cap` bytes in all; in->eof is set where the file ends */
static int fill_chunk(input_t *in, uint8_t *buf, size_t *have_io, size_t cap) {
    size_t have = *have_io;
    if (in->eof || have >= cap) return UTREE_OK;
    if (in->gz) {                                 /* opt-in formats: zlib reads plain and gzip input alike */
        size_t want = cap - have, done = 0;
        while (done < want) {
            int r = gzread(in->gz, buf + have + done, (unsigned)(want - done > (1u << 30) ? (1u << 30) : want - done));
            if (r < 0) return UTREE_E_IO;
            if (r == 0) { in->eof = 1; break; }
            done += (size_t)r;
        }
        have += done;
    } else {
        /* parallel pread: the page-cache copy is the cost; several threads stream it */
        size_t want = cap - have;
        ssize_t got[READ_THREADS];
        int T = READ_THREADS;
        const off_t file_pos = in->pos;
        const int fd = in->fd;
#pragma omp parallel for num_threads(T) schedule(static, 1)
        for (int t = 0; t < T; ++t) {
            size_t a = want * (size_t)t / (size_t)T, b = want * (size_t)(t + 1) / (size_t)T, done = 0;
            got[t] = 0;
            while (done < b - a) {
                ssize_t r = pread(fd, buf + have + a + done, b - a - done, file_pos + (off_t)(a + done));
                if (r < 0) { got[t] = -1; break; }
                if (r == 0) break;
                done += (size_t)r; got[t] = (ssize_t)done;
            }
        }
        size_t total = 0;
        for (int t = 0; t < T; ++t) {
            if (got[t] < 0) return UTREE_E_IO;
            size_t seg = want * (size_t)(t + 1) / (size_t)T - want * (size_t)t / (size_t)T;
            total += (size_t)got[t];
            if ((size_t)got[t] < seg) { in->eof = 1; break; }       /* short segment: end of file inside it */
        }
        have += total; in->pos += (off_t)total;
    }
    *have_io = have;
    return UTREE_OK;
}

static int frame_chunk(int format, const frames_t *f, size_t have, int final, size_t max_reads, size_t *nr, size_t *used, utree_fasta_error *ferr) {
    return format != UTREE_INPUT_REFERENCE
        ? utree_reads_frame(f->buf, have, final, format, max_reads, f->seq_off, f->seq_len, f->name_off, f->name_len, nr, used, ferr)
        : utree_fasta_frame(f->buf, have, final, max_reads, f->seq_off, f->seq_len, f->name_off, f->name_len, nr, used, ferr);
}

static void resolve_format(reader_t *R, const uint8_t *buf, size_t have) {
    if (have && R->input_format == UTREE_INPUT_AUTO) R->input_format = buf[0] == '@' ? UTREE_INPUT_FASTQ : UTREE_INPUT_FASTA_MULTILINE;
}

int reader_step(reader_t *R, frames_t *f, reader_outcome *o) {
    input_t *in = &R->in[0];
    memset(o, 0, sizeof *o);
    if (R->carry) memmove(f->buf, R->carry_src, R->carry);
    size_t have = R->carry;
    double t0 = now_s();
    if (fill_chunk(in, f->buf, &have, R->chunk)) return UTREE_E_IO;
    double t1 = now_s();
    const int eof = in->eof;
    o->have = have;
    resolve_format(R, f->buf, have);
    if (have) {
        o->frame_rc = frame_chunk(R->input_format, f, have, eof, R->max_reads, &o->nr, &o->used, &o->ferr);
        if (o->frame_rc != UTREE_OK && o->frame_rc != UTREE_E_FASTA) return o->frame_rc;
        if (o->frame_rc == UTREE_OK && !o->nr && !o->used && !eof) {
            o->frame_rc = UTREE_E_FASTA; o->ferr.code = 5; o->ferr.read_index = 0;   /* a line pair larger than a chunk */
        }
    }
    o->t_read = t1 - t0; o->t_frame = now_s() - t1;
    R->carry = have - o->used; R->carry_src = f->buf + o->used;
    if (o->frame_rc == UTREE_E_FASTA) { R->carry = 0; in->eof = 1; }
    if (in->eof && !R->carry) o->last = 1;
    if (in->eof && R->carry && o->frame_rc == UTREE_OK && o->used == 0 && o->nr == 0) { o->last = 1; R->carry = 0; }
    return UTREE_OK;
}

/* ---- paired input --------------------------------------------------------------------------------
 * Both inputs are framed by the chosen format's framing; a slot commits the pairs BOTH of its buffers hold and the rest of each file goes to
 * the next slot, so the two buffers of a slot always begin at the same pair whatever the lengths of the files' headers.  Interleaved input
 * is one file whose records 2i and 2i+1 are pair i; an odd record at the end of a slot is carried. */

/* Multi-line FASTA was compacted in place when it was framed, so a framed record is written out again as header line + sequence + '\n'
 * (at most one byte more than it took: the file's last line may lack its newline; the buffers have 64 bytes to spare); the other formats'
 * bytes stand as they were read and are framed again. */
static size_t carry_over(uint8_t *dst, const carry_t *c, int format) {
    size_t w = 0;
    if (!c->buf) return 0;
    if (format == UTREE_INPUT_FASTA_MULTILINE) {
        for (size_t r = c->from; r < c->nr; ++r) {
            const size_t a = (size_t)c->name_off[r] - 1, b = (size_t)c->seq_off[r] + c->seq_len[r];
            memmove(dst + w, c->buf + a, b - a); w += b - a;
            dst[w++] = '\n';
        }
        memmove(dst + w, c->buf + c->used, c->have - c->used); w += c->have - c->used;
    } else {
        const size_t a = c->from < c->nr ? (size_t)c->name_off[c->from] - 1 : c->used;
        memmove(dst, c->buf + a, c->have - a); w = c->have - a;
    }
    return w;
}

/* How a slot of a paired search ends, once its np pairs are known.  Per input k: the slot commits done[k] of the nr[k] records framed in its
 * buffer of have[k] bytes, of which framing took used[k]; frc[k] / fe[k]: a malformed record stopped the framing (it is record nr[k] of the
 * buffer); recs[k]: records the slots before committed.  In this order:
 *   1. a malformed record that is the NEXT record of its file (interleaved: or the mate of the next) ends the search with its own code; its
 *      number counts that file's records.  One further on is carried and met again;
 *   2. one file is used up -- end of file, nothing left in the buffer -- and the other's buffer holds more: UTREE_E_PAIRS (interleaved: the
 *      file is used up with an odd record left); the slot's complete pairs go through the stages first;
 *   3. every file is used up: the last slot;
 *   4. no pair, and a FULL buffer that holds no complete record (interleaved: no two): "sequence too long", as for single reads;
 *   else the next slot goes on behind done[k] (a file that ended exactly at a buffer's end is seen to be used up there). */
static void pairs_verdict(reader_t *R, reader_outcome *o, size_t np, const size_t *done, const size_t *nr, const size_t *used, const size_t *have,
                          const int *frc, const utree_fasta_error *fe) {
    const int two = R->paired == PAIRS_TWO_FILES, nin = two ? 2 : 1;
    const uint64_t *recs = R->recs;
    int rest[2] = {0, 0}, over[2] = {0, 0};                                               /* the buffer holds more of the file; the file is used up */
    for (int k = 0; k < nin; ++k) {
        rest[k] = done[k] < nr[k] || used[k] < have[k];
        over[k] = !rest[k] && R->in[k].eof;
    }
    for (int k = 0; k < nin; ++k)                                                         /* 1 */
        if (frc[k] == UTREE_E_FASTA && nr[k] - done[k] <= (two ? 0u : 1u)) {
            o->frame_rc = UTREE_E_FASTA; o->ferr = fe[k]; o->ferr.read_index += recs[k];   /* (the framing counts from the buffer's first record) */
            return;
        }
    if (two && over[0] != over[1] && rest[over[0] ? 1 : 0]) {                             /* 2 */
        const int k = over[0] ? 0 : 1;                                                    /* the shorter file */
        o->frame_rc = UTREE_E_PAIRS;
        snprintf(R->msg_pairs, R->msg_cap, "paired input: %s file %s ends after %llu records, %s goes on", k ? "the mates" : "the reads",
                 k ? R->mates_path : R->reads_path, (unsigned long long)(recs[k] + done[k]), k ? R->reads_path : R->mates_path);
    } else if (!two && R->in[0].eof && used[0] >= have[0] && (nr[0] & 1)) {
        o->frame_rc = UTREE_E_PAIRS;
        snprintf(R->msg_pairs, R->msg_cap, "paired input: the interleaved file %s holds an odd number of records (%llu): its last read has no mate",
                 R->reads_path, (unsigned long long)(recs[0] + nr[0]));
    } else if (over[0] && (!two || over[1])) o->last = 1;                                 /* 3 */
    else if (!np) {                                                                       /* 4 */
        int full = 0;
        for (int k = 0; k < nin; ++k) full |= have[k] >= R->chunk && nr[k] < (two ? 1u : 2u) && (k == 0 || nr[0] > 0);   /* (the mates are framed only up to the reads' count) */
        if (full) { o->frame_rc = UTREE_E_FASTA; o->ferr.code = 5; o->ferr.read_index = R->pairs + 1; }
    }
}

int reader_pairs_step(reader_t *R, frames_t *f1, frames_t *f2, reader_outcome *o) {
    const int two = R->paired == PAIRS_TWO_FILES, nin = two ? 2 : 1;
    frames_t *f[2] = {f1, f2};
    size_t have[2] = {0, 0}, nr[2] = {0, 0}, used[2] = {0, 0};
    int frc[2] = {UTREE_OK, UTREE_OK};
    utree_fasta_error fe[2];
    memset(o, 0, sizeof *o);
    double t0 = now_s();
    for (int k = 0; k < nin; ++k) {
        have[k] = carry_over(f[k]->buf, &R->cy[k], R->input_format);
        if (fill_chunk(&R->in[k], f[k]->buf, &have[k], R->chunk)) return UTREE_E_IO;
    }
    double t1 = now_s();
    resolve_format(R, f1->buf, have[0]);
    for (int k = 0; k < nin; ++k) {
        memset(&fe[k], 0, sizeof fe[k]);
        const size_t max_reads = k ? nr[0] : R->max_reads;                                /* no more mates than reads */
        if (!have[k] || !max_reads) continue;
        frc[k] = frame_chunk(R->input_format, f[k], have[k], R->in[k].eof, max_reads, &nr[k], &used[k], &fe[k]);
        if (frc[k] != UTREE_OK && frc[k] != UTREE_E_FASTA) return frc[k];
    }
    size_t np = two ? (nr[0] < nr[1] ? nr[0] : nr[1]) : nr[0] / 2;
    if (!two)                                                                             /* records 2i, 2i+1 -> pair i (an odd last record stays where it is) */
        for (size_t r = 0; r < np; ++r) {
            f2->seq_off[r] = f1->seq_off[2 * r + 1]; f2->seq_len[r] = f1->seq_len[2 * r + 1];
            f1->seq_off[r] = f1->seq_off[2 * r]; f1->seq_len[r] = f1->seq_len[2 * r];
            f1->name_off[r] = f1->name_off[2 * r]; f1->name_len[r] = f1->name_len[2 * r];
        }
    o->have = have[0]; o->used = used[0];
    for (size_t r = 0; r < np; ++r)
        if ((uint64_t)f1->seq_len[r] + 1 + f2->seq_len[r] > LINELEN_MAX) {                 /* "sequence too long": the pairs before it are written */
            np = r; o->frame_rc = UTREE_E_FASTA; o->ferr.code = 5; o->ferr.read_index = R->pairs + r + 1;
            break;
        }
    const size_t done[2] = {two ? np : 2 * np, np};                                       /* records of each file this slot commits */
    if (o->frame_rc == UTREE_OK) pairs_verdict(R, o, np, done, nr, used, have, frc, fe);
    if (o->frame_rc != UTREE_OK) o->last = 1;
    o->nr = np;
    for (int k = 0; k < nin; ++k) {
        R->cy[k] = (carry_t){f[k]->buf, f[k]->name_off, f[k]->seq_off, f[k]->seq_len, done[k], nr[k], used[k], have[k]};
        R->recs[k] += done[k];
    }
    R->pairs += np;
    o->t_read = t1 - t0; o->t_frame = now_s() - t1;
    return UTREE_OK;
}
