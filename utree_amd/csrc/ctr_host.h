/* ctr_host.h -- private definition of utree_ctr (host side of a database). */
#ifndef UTREE_CTR_HOST_H
#define UTREE_CTR_HOST_H
#include "utree_internal.h"

struct utree_ctr {
    utree_ctr_info info;
    uint64_t hdr_W_raw, hdr_cnt_raw, hdr_I_raw;
    char *path;                 /* file the node dump is streamed from (NULL for from_memory)             */
    uint64_t records_file_off;
    void *binix_raw;            /* 2^24+1 entries at the on-disk width                                     */
    uint64_t bins_read;
    uint8_t *h_records;         /* optional host copy (from_memory)                                        */
    char *label_text;           /* file tail; labels[] point into it (TABs/newlines replaced by NUL)       */
    size_t label_text_len;
    char **labels;              /* file order = label index                                                */
    uint32_t *label_len;
    uint32_t *rank2ix, *ix2rank;/* strcmp order <-> file order                                             */
};

/* The two halves of an output line of the GG search behind the query's name (fasta.c), shared by utree_format_records and the tile lines of
 * tiles.c.  utk_record_taxon: the taxon a record prints -- the first bytes of *text, their number returned ((size_t)-1: the label is none of
 * ctr's).  utk_record_tail: "\t taxon \t found \t uix \t sl;ol \n" (itree.c:1032, 1040, 1096) at o, at most ll + UTK_RECORD_TAIL_MAX bytes;
 * returns the byte behind them. */
#define UTK_RECORD_TAIL_MAX 48
size_t utk_record_taxon(const utree_ctr *ctr, const utree_result *r, const char **text);
char *utk_record_tail(const char *lab, size_t ll, const utree_result *r, char *o);

#endif
