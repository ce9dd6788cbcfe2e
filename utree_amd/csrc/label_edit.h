/* label_edit.h -- the label edit of utree_merge_files_edit (include/utree_amd.h): the rule files (drop, keep, rename) and the edit of one
 * label text -- clade match, selection on the original text, longest rename once, rank cut.  Plain C without a device: merge.c uses it,
 * and a stand-alone program can link label_edit.c alone.  Private. */
#ifndef UTREE_LABEL_EDIT_H
#define UTREE_LABEL_EDIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { LE_KEEP = 0, LE_RENAME = 1, LE_CUT = 2, LE_DROP = 4 };                  /* le_apply: LE_DROP alone, or LE_RENAME | LE_CUT bits */

typedef struct le_rules le_rules;

/* Reads the rule files (NULL: none).  UTREE_OK, UTREE_E_IO (a file cannot be opened or read), UTREE_E_FORMAT (a malformed line),
 * UTREE_E_NOMEM; err[0 .. errn) gets the text of a failure -- it names the file and, for a malformed line, the 1-based line. */
int le_load(le_rules **out, uint32_t ranks, const char *drop_path, const char *keep_path, const char *rename_path, char *err, size_t errn);
void le_free(le_rules *R);

/* The edit of t[0 .. n): the action, and for all but LE_DROP the edited text in (*text)[0 .. *text_n) -- it points into t or into a buffer
 * of R that the next call reuses.  Every rule whose taxon matches t is marked as matched.  -1: out of memory. */
int le_apply(le_rules *R, const char *t, size_t n, const char **text, size_t *text_n);

/* the rules that no le_apply has matched, in the order drop file, keep file, rename file and line order */
uint64_t le_unmatched(const le_rules *R);
typedef void (*le_unmatched_fn)(void *ctx, const char *file, uint64_t line, const char *text, size_t text_n);
void le_each_unmatched(const le_rules *R, le_unmatched_fn fn, void *ctx);

#ifdef __cplusplus
}
#endif
#endif
