/* search_reader_asan.c -- the reader steps of the host pipeline (utree_amd/csrc/search_reader.c) as a stand-alone host program for
 * AddressSanitizer + UndefinedBehaviorSanitizer: `make -C utree_amd/csrc search-reader-asan`.  It writes small read files into a temporary
 * directory and drives reader_step / reader_pairs_step alone, alternating between two slots' buffers, at chunk sizes from two records to more
 * than the file.  What the slots commit is held against the framing of the WHOLE file in one buffer (utree_fasta_frame / utree_reads_frame),
 * and how a search ends -- the last slot, UTREE_E_PAIRS and its text, a malformed record's code and number -- against the run whose chunk
 * holds the whole file.  Records take at most 60 bytes, so that at the smallest chunk (128 bytes) two always fit and "sequence too long"
 * comes up only where a case asks for it.  No GPU, no Python.  Exit code 0: all as expected and no sanitizer report. */
#define _GNU_SOURCE
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>
#include "../include/utree_amd.h"
#include "../utree_amd/csrc/search_reader.h"

static int failures;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d (%s): %s\n", __LINE__, what, #c); ++failures; } } while (0)
static char what[320];                          /* the case under way, for the messages */

enum { REF = UTREE_INPUT_REFERENCE, FQ = UTREE_INPUT_FASTQ, ML = UTREE_INPUT_FASTA_MULTILINE };
#define MAXR 4096                               /* records a slot's arrays hold */
#define NREC 50
static const size_t CHUNKS[] = {128, 129, 191, 4096, (size_t)1 << 16};   /* the last: more than any file here */
#define NCHUNKS (sizeof CHUNKS / sizeof CHUNKS[0])

typedef struct { char p[1 << 16]; size_t n; uint64_t recs; } text_t;
static void put(text_t *t, const void *d, size_t n) {
    if (t->n + n > sizeof t->p) { fprintf(stderr, "text buffer too small\n"); exit(1); }
    memcpy(t->p + t->n, d, n); t->n += n;
}
/* "name \t sequence", by content */
static void put_rec(text_t *t, const frames_t *f, size_t r, char end) {
    put(t, f->buf + f->name_off[r], f->name_len[r]); put(t, "\t", 1);
    put(t, f->buf + f->seq_off[r], f->seq_len[r]); put(t, &end, 1);
}
static void put_pair(text_t *t, const frames_t *f1, size_t r1, const frames_t *f2, const uint8_t *buf2, size_t r2) {
    put_rec(t, f1, r1, '|');
    put(t, buf2 + f2->seq_off[r2], f2->seq_len[r2]); put(t, "\n", 1);
    ++t->recs;
}

static void frames_new(frames_t *f, size_t bytes) {
    f->buf = (uint8_t *)malloc(bytes + 64);
    f->seq_off = (uint64_t *)malloc(MAXR * 8); f->name_off = (uint64_t *)malloc(MAXR * 8); f->rel_off = NULL;
    f->seq_len = (uint32_t *)malloc(MAXR * 4); f->name_len = (uint32_t *)malloc(MAXR * 4);
    if (!f->buf || !f->seq_off || !f->name_off || !f->seq_len || !f->name_len) { perror("malloc"); exit(1); }
}
static void frames_del(frames_t *f) { free(f->buf); free(f->seq_off); free(f->name_off); free(f->seq_len); free(f->name_len); }

/* ---- the files ------------------------------------------------------------------------------------------------------------------------- */
typedef struct { uint8_t p[1 << 15]; size_t n; } bytes_t;
enum { GOOD = 0, BAD, LONG };

/* record `idx` of file `who` (0: the reads, short headers; 1: the mates, longer ones): 1 .. 44 bases (FASTQ: 1 .. 22), multi-line FASTA in lines
 * of 16.  BAD: a header without its lead byte (reference framing: code 2) or a FASTQ separator that is no '+' (code 3); LONG: 200 bases */
static void add_record(bytes_t *b, int format, int who, unsigned idx, int kind) {
    static const char acgt[] = "ACGT";
    unsigned x = (idx + 1) * 2654435761u ^ (who ? 0x9E3779B9u : 0x7F4A7C15u);
    unsigned len = kind == LONG ? 200 : 1 + (x >> 8) % (format == FQ ? 22 : 44);
    char *o = (char *)b->p + b->n;
    const char lead = format == FQ ? '@' : '>';
    o += sprintf(o, who ? "%cmate%u/2\n" : "%cr%u\n", kind == BAD && format != FQ ? 'X' : lead, idx);
    for (unsigned i = 0; i < len; ++i) {
        x = x * 1664525u + 1013904223u;
        *o++ = acgt[x >> 30];
        if (format == ML && i % 16 == 15 && i + 1 < len) *o++ = '\n';
    }
    *o++ = '\n';
    if (format == FQ) {
        o += sprintf(o, "%c\n", kind == BAD ? '-' : '+');
        for (unsigned i = 0; i < len; ++i) *o++ = (char)('#' + i % 40);
        *o++ = '\n';
    }
    b->n = (size_t)(o - (char *)b->p);
    if (b->n > sizeof b->p - 512) { fprintf(stderr, "file buffer too small\n"); exit(1); }
}
/* n records of file `who`; record `at` (-1: none) is of `kind` */
static void make_file(bytes_t *b, int format, int who, unsigned n, int at, int kind) {
    b->n = 0;
    for (unsigned i = 0; i < n; ++i) add_record(b, format, who, i, (int)i == at ? kind : GOOD);
}
/* n records, alternately of the reads and of the mates */
static void make_interleaved(bytes_t *b, int format, unsigned n, int at, int kind) {
    b->n = 0;
    for (unsigned i = 0; i < n; ++i) add_record(b, format, (int)(i & 1), i / 2, (int)i == at ? kind : GOOD);
}

static char dir[64];
static const char *save(const char *name, const bytes_t *b, int gzip) {
    static char paths[4][128];
    static int turn;
    char *p = paths[turn++ & 3];
    snprintf(p, 128, "%s/%s", dir, name);
    if (gzip) {
        gzFile g = gzopen(p, "wb");
        if (!g || gzwrite(g, b->p, (unsigned)b->n) != (int)b->n || gzclose(g) != Z_OK) { perror(p); exit(1); }
    } else {
        FILE *f = fopen(p, "wb");
        if (!f || fwrite(b->p, 1, b->n, f) != b->n || fclose(f)) { perror(p); exit(1); }
    }
    return p;
}

/* the whole file framed in one buffer: its records into *f (the caller's to delete) */
static size_t frame_whole(const bytes_t *b, int format, frames_t *f) {
    size_t nr = 0, used = 0;
    utree_fasta_error e;
    frames_new(f, b->n);
    memcpy(f->buf, b->p, b->n);
    const int rc = format == REF ? utree_fasta_frame(f->buf, b->n, 1, MAXR, f->seq_off, f->seq_len, f->name_off, f->name_len, &nr, &used, &e)
                                 : utree_reads_frame(f->buf, b->n, 1, format, MAXR, f->seq_off, f->seq_len, f->name_off, f->name_len, &nr, &used, &e);
    CHECK(rc == UTREE_OK && used == b->n);
    return nr;
}

/* ---- one search's reader: the steps until the input ends, the slots alternating ------------------------------------------------------- */
typedef struct {
    int rc;                                     /* a step's own return code                                  */
    int frame_rc, last; utree_fasta_error ferr; /* of the slot that ended the run                            */
    char msg[512];
    text_t got;                                 /* the committed records (pairs)                             */
    unsigned slots;
} run_t;

static void run(int paired, int format, const char *p0, const char *p1, size_t chunk, run_t *o) {
    reader_t R;
    frames_t rd[2], m2[2];
    memset(&R, 0, sizeof R); memset(o, 0, sizeof *o);
    memset(m2, 0, sizeof m2);
    R.input_format = format; R.paired = paired; R.chunk = chunk; R.max_reads = MAXR;
    R.reads_path = "READS"; R.mates_path = "MATES"; R.msg_pairs = o->msg; R.msg_cap = sizeof o->msg;
    R.in[1].fd = -1;
    for (int k = 0; k < (paired == PAIRS_TWO_FILES ? 2 : 1); ++k) {
        R.in[k].fd = open(k ? p1 : p0, O_RDONLY);
        if (R.in[k].fd < 0) { perror(k ? p1 : p0); exit(1); }
        if (format != REF && !(R.in[k].gz = gzdopen(dup(R.in[k].fd), "rb"))) { perror("gzdopen"); exit(1); }
    }
    for (int i = 0; i < 2; ++i) {
        frames_new(&rd[i], chunk);
        if (paired) frames_new(&m2[i], paired == PAIRS_TWO_FILES ? chunk : 0);
    }
    for (;; ++o->slots) {
        frames_t *f1 = &rd[o->slots & 1], *f2 = &m2[o->slots & 1];
        reader_outcome out;
        if (o->slots > 100000) { CHECK(!"the reader makes no progress"); break; }
        o->rc = paired ? reader_pairs_step(&R, f1, f2, &out) : reader_step(&R, f1, &out);
        if (o->rc) break;
        CHECK(out.nr <= MAXR && out.used <= out.have && out.have <= chunk + 1);
        for (size_t r = 0; r < out.nr; ++r) {
            if (paired) put_pair(&o->got, f1, r, f2, paired == PAIRS_TWO_FILES ? f2->buf : f1->buf, r);
            else { put_rec(&o->got, f1, r, '\n'); ++o->got.recs; }
        }
        o->frame_rc = out.frame_rc; o->last = out.last; o->ferr = out.ferr;
        if (out.last || out.frame_rc != UTREE_OK) { ++o->slots; break; }
    }
    for (int i = 0; i < 2; ++i) { frames_del(&rd[i]); if (paired) frames_del(&m2[i]); }
    for (int k = 0; k < 2; ++k) {
        if (R.in[k].gz) gzclose(R.in[k].gz);
        if (R.in[k].fd >= 0) close(R.in[k].fd);
    }
}

static int same_text(const text_t *a, const text_t *b) { return a->n == b->n && a->recs == b->recs && !memcmp(a->p, b->p, a->n); }
/* two runs ended the same way: code, record number, text, and the records committed in front */
static int same_end(const run_t *a, const run_t *b) {
    return a->rc == b->rc && a->frame_rc == b->frame_rc && a->ferr.code == b->ferr.code && a->ferr.read_index == b->ferr.read_index &&
           !strcmp(a->msg, b->msg) && same_text(&a->got, &b->got);
}

static const char *fmt_name(int f) { return f == REF ? "reference" : f == FQ ? "fastq" : "multi-line"; }
static const char *mode_name(int m) { return m == PAIRS_NONE ? "single" : m == PAIRS_TWO_FILES ? "two files" : "interleaved"; }

static bytes_t b0, b1;
static run_t r, big, gz;
static text_t want;

/* every chunk size ends as the chunk that holds the whole file does: *big is that run, checked by the caller */
static void same_at_every_chunk(int paired, int format, const char *p0, const char *p1) {
    char base[208];
    snprintf(base, sizeof base, "%.200s", what);
    for (size_t c = 0; c + 1 < NCHUNKS; ++c) {
        snprintf(what, sizeof what, "%s, chunk %zu", base, CHUNKS[c]);
        run(paired, format, p0, p1, CHUNKS[c], &r);
        CHECK(same_end(&r, &big));
    }
}

int main(void) {
    strcpy(dir, "/tmp/search_reader_asan.XXXXXX");
    if (!mkdtemp(dir)) { perror("mkdtemp"); return 1; }
    static const int formats[] = {REF, ML, FQ}, modes[] = {PAIRS_NONE, PAIRS_TWO_FILES, PAIRS_INTERLEAVED};

    /* committed records and pairs: their concatenation over the slots is the framing of the whole file(s); the last slot says so */
    for (int fi = 0; fi < 3; ++fi) for (int mi = 0; mi < 3; ++mi) {
        const int format = formats[fi], mode = modes[mi];
        frames_t w0, w1;
        size_t n0, n1 = 0;
        snprintf(what, sizeof what, "%s, %s", mode_name(mode), fmt_name(format));
        if (mode == PAIRS_INTERLEAVED) make_interleaved(&b0, format, 2 * NREC, -1, GOOD); else make_file(&b0, format, 0, NREC, -1, GOOD);
        make_file(&b1, format, 1, NREC, -1, GOOD);
        const char *p0 = save("reads", &b0, 0), *p1 = save("mates", &b1, 0);
        n0 = frame_whole(&b0, format, &w0);
        if (mode == PAIRS_TWO_FILES) n1 = frame_whole(&b1, format, &w1);
        want.n = 0; want.recs = 0;
        CHECK(n0 == (mode == PAIRS_INTERLEAVED ? 2 * NREC : NREC) && (mode != PAIRS_TWO_FILES || n1 == NREC));
        for (size_t i = 0; i < NREC; ++i) {
            if (mode == PAIRS_NONE) { put_rec(&want, &w0, i, '\n'); ++want.recs; }
            else if (mode == PAIRS_TWO_FILES) put_pair(&want, &w0, i, &w1, w1.buf, i);
            else put_pair(&want, &w0, 2 * i, &w0, w0.buf, 2 * i + 1);
        }
        frames_del(&w0);
        if (mode == PAIRS_TWO_FILES) frames_del(&w1);
        const char *g0 = NULL, *g1 = NULL;
        if (format != REF) { g0 = save("reads.gz", &b0, 1); g1 = save("mates.gz", &b1, 1); }   /* zlib reads the opt-in formats, plain and gzip alike */
        for (size_t c = 0; c < NCHUNKS; ++c) {
            snprintf(what, sizeof what, "%s, %s, chunk %zu", mode_name(mode), fmt_name(format), CHUNKS[c]);
            run(mode, format, p0, p1, CHUNKS[c], &r);
            CHECK(r.rc == UTREE_OK && r.frame_rc == UTREE_OK && r.last == 1 && !r.msg[0]);
            CHECK(r.got.recs == NREC && same_text(&r.got, &want));
            if (c + 1 == NCHUNKS) CHECK(r.slots == 1);
            if (g0) {
                run(mode, format, g0, g1, CHUNKS[c], &gz);
                CHECK(gz.last == 1 && gz.slots == r.slots && same_end(&gz, &r));
            }
        }
    }

    /* a file that runs out in front of the other, an odd interleaved file: UTREE_E_PAIRS behind the complete pairs, the same text at every chunk size */
    for (int fi = 0; fi < 3; ++fi) for (int k = 0; k < 3; ++k) {
        const int format = formats[fi], mode = k == 2 ? PAIRS_INTERLEAVED : PAIRS_TWO_FILES;
        snprintf(what, sizeof what, "%s, %s", k == 0 ? "mates one short" : k == 1 ? "mates one long" : "interleaved, odd", fmt_name(format));
        if (k == 2) make_interleaved(&b0, format, 2 * NREC - 1, -1, GOOD); else make_file(&b0, format, 0, NREC, -1, GOOD);
        make_file(&b1, format, 1, k == 0 ? NREC - 1 : NREC + 1, -1, GOOD);
        const char *p0 = save("reads", &b0, 0), *p1 = save("mates", &b1, 0);
        run(mode, format, p0, p1, CHUNKS[NCHUNKS - 1], &big);
        CHECK(big.rc == UTREE_OK && big.frame_rc == UTREE_E_PAIRS && big.got.recs == (k == 1 ? NREC : NREC - 1));
        if (k == 0) CHECK(!strcmp(big.msg, "paired input: the mates file MATES ends after 49 records, READS goes on"));
        if (k == 1) CHECK(!strcmp(big.msg, "paired input: the reads file READS ends after 50 records, MATES goes on"));
        if (k == 2) CHECK(!strcmp(big.msg, "paired input: the interleaved file READS holds an odd number of records (99): its last read has no mate"));
        same_at_every_chunk(mode, format, p0, p1);
        if (format != REF) {
            const char *g0 = save("reads.gz", &b0, 1), *g1 = save("mates.gz", &b1, 1);
            run(mode, format, g0, g1, 191, &gz);
            CHECK(same_end(&gz, &big));
        }
    }

    /* a malformed record as the first, a middle and the last record of either file: its own code, its number in its file, the pairs in front of it */
    for (int fi = 0; fi < 3; fi += 2) for (int who = 0; who < 3; ++who) for (int at = 0; at < 3; ++at) {
        const int format = formats[fi], mode = who == 2 ? PAIRS_INTERLEAVED : PAIRS_TWO_FILES;
        const int n = who == 2 ? 2 * NREC : NREC, pos = at == 0 ? 0 : at == 1 ? (who == 2 ? 51 : 23) : n - 1;
        snprintf(what, sizeof what, "malformed record %d of %s, %s", pos, who == 0 ? "the reads" : who == 1 ? "the mates" : "the interleaved file", fmt_name(format));
        if (who == 2) make_interleaved(&b0, format, 2 * NREC, pos, BAD); else make_file(&b0, format, 0, NREC, who == 0 ? pos : -1, BAD);
        make_file(&b1, format, 1, NREC, who == 1 ? pos : -1, BAD);
        const char *p0 = save("reads", &b0, 0), *p1 = save("mates", &b1, 0);
        run(mode, format, p0, p1, CHUNKS[NCHUNKS - 1], &big);
        CHECK(big.rc == UTREE_OK && big.frame_rc == UTREE_E_FASTA && big.ferr.code == (format == FQ ? 3 : 2) && big.ferr.read_index == (uint64_t)pos + 1);
        CHECK(big.got.recs == (uint64_t)(who == 2 ? pos / 2 : pos) && !big.msg[0]);
        same_at_every_chunk(mode, format, p0, p1);
    }

    /* a record longer than the chunk: "sequence too long" for the pair it belongs to, behind the pairs in front of it */
    for (int who = 0; who < 2; ++who) {
        snprintf(what, sizeof what, "a 200-byte record in %s, chunk 128", who ? "the mates" : "the reads");
        make_file(&b0, REF, 0, NREC, who == 0 ? 10 : -1, LONG);
        make_file(&b1, REF, 1, NREC, who == 1 ? 10 : -1, LONG);
        run(PAIRS_TWO_FILES, REF, save("reads", &b0, 0), save("mates", &b1, 0), 128, &r);
        CHECK(r.rc == UTREE_OK && r.frame_rc == UTREE_E_FASTA && r.ferr.code == 5 && r.got.recs == 10 && r.ferr.read_index == r.got.recs + 1);
    }

    char cmd[160];
    snprintf(cmd, sizeof cmd, "rm -rf %s", dir);
    if (system(cmd)) ++failures;
    if (failures) { fprintf(stderr, "search_reader_asan: %d checks failed\n", failures); return 1; }
    puts("search_reader_asan: ok");
    return 0;
}
