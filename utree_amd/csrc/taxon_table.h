/* taxon_table.h -- the per-taxon table every report file is (taxon_table.c), private. */
#ifndef UTREE_TAXON_TABLE_H
#define UTREE_TAXON_TABLE_H
#include <stddef.h>
#include <stdint.h>

#define UTREE_TAXON_FIGURES 3
typedef struct { const char *s; uint32_t len; uint64_t own[UTREE_TAXON_FIGURES], clade[UTREE_TAXON_FIGURES]; } utree_taxon_row;

/* Writes `header` (the file's two '#' lines) and one line "<taxon>\t<own figures>\t<clade figures>\n" per row to `path`.  `t` holds n input
 * texts with their first n_fig own figures (sorted and merged in place).  Rows: every text whose figure `key` is > 0 and every ';'-prefix of
 * one, in unsigned bytewise order (shorter first on a tie).  A row's own figures are those of the inputs of exactly that text, its clade
 * figures the sum over ALL inputs whose text is the row's or begins with it + ';'.  UTREE_OK, UTREE_E_NOMEM or UTREE_E_IO. */
int utree_taxon_table_write(utree_taxon_row *t, size_t n, int n_fig, int key, const char *header, const char *path);

#endif
