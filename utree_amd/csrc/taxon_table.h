/* taxon_table.h -- the per-taxon table every report file is (taxon_table.c), private. */
#ifndef UTREE_TAXON_TABLE_H
#define UTREE_TAXON_TABLE_H
#include <stddef.h>
#include <stdint.h>

/* unsigned bytewise order, the shorter text first on a tie: the order of every report's rows and of a matrix's columns */
int utree_text_cmp(const void *a, uint64_t la, const void *b, uint64_t lb);

#define UTREE_TAXON_FIGURES 7
typedef struct { const char *s; uint32_t len; uint64_t own[UTREE_TAXON_FIGURES], clade[UTREE_TAXON_FIGURES]; } utree_taxon_row;

/* Writes `header` (the file's two '#' lines) and one line "<taxon>\t<own figures>\t<clade figures>\n" per row to `path`.  `t` holds n input
 * texts with their first n_fig own figures (sorted and merged in place).  Rows: every text whose figure `key` is > 0 and every ';'-prefix of
 * one, in unsigned bytewise order (shorter first on a tie).  A row's own figures are those of the inputs of exactly that text, its clade
 * figures the sum over ALL inputs whose text is the row's or begins with it + ';'.  UTREE_OK, UTREE_E_NOMEM or UTREE_E_IO. */
int utree_taxon_table_write(utree_taxon_row *t, size_t n, int n_fig, int key, const char *header, const char *path);
/* The same with n_own own figures per line followed by the clade figures of the first n_clade of them (n_clade <= n_own), and with key < 0
 * for "every input text is a row" (the database compare: seven own figures, clades of its first two). */
int utree_taxon_table_write_wide(utree_taxon_row *t, size_t n, int n_own, int n_clade, int key, const char *header, const char *path);
/* The same with the clade figures picked: clade column q sums own figure clade_of[q] (the database inspection: five own figures, clades of
 * its first and its last). */
int utree_taxon_table_write_pick(utree_taxon_row *t, size_t n, int n_own, const int *clade_of, int n_clade, int key, const char *header, const char *path);

/* The per-sample matrix (the layouts are in include/utree_amd.h: utree_samples_write, utree_sredist_write): a column per sample, a row per taxon. */
typedef struct { const uint8_t *s; uint64_t len; uint64_t reads, uncl; } utree_matrix_col;     /* a sample: its id, reads, unclassified reads  */
typedef struct { const char *name; const uint64_t *v; } utree_matrix_extra;                   /* a further "# name" header row: v[column]     */
typedef struct { const char *s; uint32_t len; uint32_t col; uint64_t reads; } utree_matrix_cell;

/* Writes `header` + "\tsamples\t<columns>" (the file's first line), the rows "# taxon" (ids; TAB, CR and backslash escaped), "# reads", "# unclassified"
 * and the n_extra further ones, then one row per distinct text of the q entries (any order; sorted and merged by (text, column) in place), a 0 where
 * a sample has none.  The columns come in the caller's order -- what `col` and `v` index -- and are written in the order of their ids; columns of
 * one id are one column, their figures added up (`merge`), or refused.  UTREE_E_ARG, and no file, for that, for an entry that names no column and
 * for a column whose entries do not sum to its reads - unclassified; UTREE_E_NOMEM, UTREE_E_IO. */
int utree_sample_matrix_write(const char *header, const utree_matrix_col *col, size_t S, int merge, const utree_matrix_extra *extra, size_t n_extra,
                              utree_matrix_cell *e, size_t q, const char *path);

#endif
