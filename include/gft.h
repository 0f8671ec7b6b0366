/* gft.h -- C ABI of libgft.so: MI355X (gfx950) implementation of gofindthem's ProcessText hot path.
 *
 * Drop-in boundary for the reference's Go interface finder.SubstringEngine
 * (finder/substringEngine.go:11-18) and for the per-document solve loop of finder.Finder.ProcessText
 * (finder/finder.go:139-215).  Plain pointers and sizes only: a cgo shim binds these directly (see
 * INTEGRATION.md).  Paths cited below are relative to the reference repository.
 *
 * Conventions
 *   - every function returns GFT_OK (0) or a negative gft_status; gft_last_error() gives the message.  (One positive
 *     value exists, GFT_W_NO_RCCL, a warning of gft_engine_create_multi.)  No C++ exception ever crosses this boundary:
 *     every entry point translates whatever its host code throws into GFT_E_NOMEM / GFT_E_INTERNAL.
 *   - the caller owns its input buffers; the library never retains them after a call returns (cgo rule).
 *   - "blob + offsets": n byte strings are passed as one contiguous blob and n+1 uint64 offsets.
 *   - term ids index the engine's own dictionary order: unique terms sorted bytewise (the reference's
 *     DictIndex is Go-map-iteration order, i.e. meaningless across runs: substringEngine.go:99-104).
 *   - positions are byte offsets into the (already case-folded) text, like Match.Position
 *     (finder/finder.go:11-14), uint32 per document.
 *   - match order inside one document is the reference engine's emission order: end offset ascending,
 *     then term length descending (node first, then its dictionary-suffix chain).
 *   - every entry point takes the handle's own mutex: a built engine / finder may be shared between threads (goroutines),
 *     calls on one handle are serialised; result buffers the library owns (gft_scan, gft_finder_expression ...) stay valid
 *     until the NEXT call on the same handle, so a caller that shares a handle copies them before releasing its own lock.
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with GFT_E_HIP.
 */
#ifndef GFT_H
#define GFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gft_status {
    GFT_OK = 0,
    GFT_E_INVALID = -1,     /* bad argument */
    GFT_E_NOT_BUILT = -2,   /* gft_build / gft_set_programs has not been called */
    GFT_E_HIP = -3,         /* HIP runtime error (message has the HIP error string) */
    GFT_E_UNSUPPORTED = -4, /* input exceeds a documented limit of the device path */
    GFT_E_PARSE = -5,       /* DSL error; message is the reference parser's error text */
    GFT_E_ENGINE = -6,      /* an injected engine (host mirror) reported an error */
    GFT_E_NOMEM = -7,       /* the host side ran out of memory (std::bad_alloc / a container beyond max_size) */
    GFT_E_INTERNAL = -8,    /* any other C++ exception on the host side: caught at the ABI, never propagated (the reference
                             * returns errors, it does not panic: finder/finder.go:149-158) */
    GFT_W_NO_RCCL = 1       /* gft_engine_create_multi only, a WARNING: the handle is valid and complete, but RCCL could not
                             * be loaded or ncclCommInitAll failed (gft_last_error says why) -- gft_process_device_multi
                             * gathers the bitmaps with device-to-device copies instead of ncclSend / ncclRecv */
} gft_status;

/* gft_build flags */
#define GFT_POS_START 0u /* Position = offset of the first byte of the match (default) */
#define GFT_POS_END 1u   /* Position = offset of the last byte of the match */
/* gft_scan / gft_process flags */
#define GFT_FOLD_ASCII 1u /* lower-case A-Z while reading the text (finder.go:140-142 for ASCII input).  This IS
                           * strings.ToLower only while the text is ASCII: the kernels notice bytes >= 0x80 on their way
                           * (gft_last_nonascii), and the finder entry points then lower such a batch in full first
                           * (gft_to_lower_device) and scan it again */

#define GFT_SCAN_UNIQUE 2u /* gft_scan / gft_scan_device: CloudflareEngine's output instead of CloudflareForkEngine's
                            * (finder/substringEngine.go:77-86): every term that occurs in a document once, in the order
                            * of its first occurrence, every pos 0 -- enough for expressions without INORD */

#define GFT_POS_RUNES 4u   /* gft_scan / gft_scan_device: AnknownEngine's positions (finder/substringEngine.go:44-53 searches
                            * []rune(text) and reports m.Pos): every pos is the number of RUNES in front of the match instead of
                            * the number of bytes, under Go's decoder (an invalid byte is one U+FFFD of width 1).  The match SET
                            * is the byte-level one, and a match that begins inside a rune counts that rune as in front of it;
                            * GFT_POS_START engines only; ignored together with GFT_SCAN_UNIQUE (pos 0) */

typedef struct gft_engine gft_engine;

/* ---- lifetime ------------------------------------------------------------------------------------- */
/* device = HIP device ordinal, or -1 for the calling thread's current device. */
int gft_engine_create(gft_engine** out, int device);
void gft_engine_destroy(gft_engine* e);
const char* gft_last_error(const gft_engine* e);
/* Run all work of this engine on an existing HIP stream (hipStream_t passed as void*).  NULL = a stream of the
 * engine's own, created blocking, i.e. ordered with the legacy default stream: device buffers produced there (torch's
 * default stream, plain hipMemcpy) can be handed to the *_device entry points without an explicit synchronisation.
 * Every entry point returns after its work has completed. */
int gft_set_stream(gft_engine* e, void* hip_stream);
/* Leave `margin` compute units free of this engine's kernels (default 0; environment: GFT_CU_MARGIN).  The scan and solver
 * kernels are persistent -- one workgroup per CU that holds the CU's whole LDS for the length of the launch --, so a kernel
 * of somebody else's (RCCL's send / receive kernels when the bitmap gather of batch i travels beside batch i + 1, bench.py
 * N > 1) finds no CU until they exit and then keeps the next launch's workgroups waiting.  With a margin those kernels
 * always find room; the batch's kernels run on n_cus - margin CUs.  Not while batches are in flight. */
int gft_set_cu_margin(gft_engine* e, uint32_t margin);

/* ---- SubstringEngine.BuildEngine (finder/substringEngine.go:98-106) ----------------------------------- */
/* Receives the full keyword set (already lower-cased by the DSL parser when case-insensitive,
 * dsl/parser.go:79-81).  Copies, sorts, de-duplicates, compiles the automaton and uploads it.
 * What an error leaves behind: the tables are compiled on the host first and the scan kernel is chosen for them
 * (csrc/table_set.cpp), and a refusal there -- a null argument, a term_off that does not ascend, a keyword longer than 7 424
 * bytes, an automaton too large, a GFT_SCAN_KERNEL that this library was built without -- returns with the handle untouched:
 * the dictionary installed before, if any, stays installed with its programs, and gft_scan* / gft_process* go on answering
 * from it.  An error after that, while the new tables are copied to the device, leaves a handle without a dictionary:
 * gft_scan* / gft_process* answer GFT_E_NOT_BUILT until a gft_build or gft_import_tables call succeeds.  A successful call
 * drops the programs (slots refer to the dictionary): gft_set_programs must be called again. */
int gft_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags);
uint32_t gft_n_terms(const gft_engine* e);  /* unique terms */
uint32_t gft_n_states(const gft_engine* e); /* automaton states incl. root */
/* term_id -> bytes of the term (pointer valid until the next gft_build / destroy) */
int gft_term(const gft_engine* e, uint32_t term_id, const uint8_t** ptr, uint32_t* len);
/* bytes of a term -> term_id, or -1 if it is not in the dictionary */
int64_t gft_term_id(const gft_engine* e, const uint8_t* term, uint32_t len);

/* Compiled tables of the current dictionary as one blob (compiling a 100 k-term dictionary costs
 * ~0.6 s of host time; a blob is installed with a copy and an upload).  gft_export_tables writes into out (cap bytes) and
 * the size into *needed (GFT_E_INVALID when cap is too small); gft_import_tables is equivalent to the gft_build call that
 * produced the blob (same terms, ids and flags), and what an error leaves behind is the same: a blob that is refused -- null,
 * truncated, corrupt, written by another library version, inconsistent in itself, or one of gft_build's refusals -- returns
 * with the handle untouched, an error while the tables are copied to the device leaves a handle that answers
 * GFT_E_NOT_BUILT.  Blobs are tied to the library version that wrote them; the library reads back every blob it writes. */
int gft_export_tables(const gft_engine* e, uint8_t* out, uint64_t cap, uint64_t* needed);
int gft_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len);

/* ---- SubstringEngine.FindSubstrings (finder/substringEngine.go:110-119), batched ------------------------ */
/* CSR result: matches of document d are [match_off[d], match_off[d+1]).  Buffers are library-owned and stay
 * valid until the next call on the same engine. */
typedef struct gft_matches {
    uint64_t n_docs;
    uint64_t n_matches;
    const uint64_t* match_off; /* n_docs + 1 */
    const uint32_t* term_id;   /* n_matches */
    const uint32_t* pos;       /* n_matches */
} gft_matches;

/* Host buffers in, host buffers out (the cgo path).  One document == one FindSubstrings call. */
int gft_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
             gft_matches* out);
/* Device-resident variant: text_blob / doc_off already live in HBM on the engine's device; the returned
 * pointers are DEVICE pointers (n_docs / n_matches are host values).  Where the text lies: d_text_blob needs no alignment and
 * d_doc_off[0] may be non-zero -- a caller's buffer at any address, a bucket's run inside the blob of gft_route_docs_device.  The
 * bytes [0, d_doc_off[0]) in front of the first document must be readable, and d_text_blob must be readable for 64 bytes past
 * d_doc_off[n_docs] (vector loads); what those bytes hold never changes the answer, neither the matches nor gft_last_nonascii --
 * not the other half of a keyword that a document border cuts, not the other half of a rune, not a neighbouring bucket's text
 * (tests/test_gpu_placement.py).  The same holds for gft_scan's host buffers: [0, doc_off[n_docs]) is uploaded as it is and
 * nothing behind it is read. */
int gft_scan_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                    uint32_t flags, gft_matches* out_dev);

/* ---- Expression programs: the solver half (dsl/expression.go:60-142, finder/finder.go:199-215) ---------- */
/* An expression is a postfix program of uint32 words, produced from the dsl.Expression tree by the host
 * side (gft_finder_* below, or the Go shim).  Word = opcode << 28 | operand.
 *   GFT_OP_UNIT  operand = slot.  Slots [0, n_terms) are dictionary term ids; slots [n_terms, n_terms+n_extra)
 *                are "extra" literals whose matches the caller supplies (regex terms, finder/regexEngine.go).
 *   GFT_OP_AND / GFT_OP_OR   binary;  GFT_OP_NOT unary;  GFT_OP_INORD unary (closes an INORD(...) group).
 *   operand bit 0 of AND/OR/UNIT-less ops is unused; UNIT/AND/OR words inside an INORD group carry
 *   GFT_INORD_FLAG (bit 27) == dsl.Expression.Inord. */
#define GFT_OP_UNIT 1u
#define GFT_OP_AND 2u
#define GFT_OP_OR 3u
#define GFT_OP_NOT 4u
#define GFT_OP_INORD 5u
#define GFT_INORD_FLAG (1u << 27)
#define GFT_SLOT_MASK ((1u << 27) - 1u)

/* Limits of the DEVICE solver that the reference does not have: an INORD group with more than 8 192 (slot, threshold) pairs
 * alive at once or a pair stack deeper than 64, a fused form that nests deeper than 128 (chains nested to one side, of any
 * length, are fine: they need no stack).  An expression beyond them is accepted all the same: gft_process* solve it on the
 * host from the scan's matches (csrc/host_solve.cpp, the reference's recursion restated -- dsl/expression.go:66-142 has no
 * such limits) and put its bit into the bitmap; every other expression of the set still runs on the device.
 * Refused with GFT_E_UNSUPPORTED: 2^25 slots or more (terms + extra literals; the solver's program words carry a 25-bit
 * slot), keywords longer than 7 424 bytes (gft_build).
 * What an error leaves behind: the set is compiled on the host first (csrc/program_set.cpp), and a refusal there -- a
 * malformed program, a limit above -- returns with the handle untouched: the set installed before, if any, stays installed
 * and gft_process* go on answering from it.  An error after that, while the new set is copied to the device, leaves a handle
 * without programs: gft_process* answer GFT_E_NOT_BUILT until a gft_set_programs call succeeds. */
int gft_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs,
                     uint32_t n_extra);
uint32_t gft_n_exprs(const gft_engine* e);
/* how many of them the HOST solves for every document (host_solve: the reference's recursion, dsl/expression.go:66-142): the
 * ones beyond the device solver's limits -- an INORD group of more than 8 192 (slot, threshold) pairs alive at once or a
 * pair stack deeper than 64, a fused form that nests deeper than 128.  0 for any rule set a person would write. */
uint32_t gft_n_host_exprs(const gft_engine* e);
/* 1 when the last scan / process call on this engine ran with GFT_FOLD_ASCII over text for which lower-casing A-Z is
 * not provably the whole of strings.ToLower (finder/finder.go:140-142): it holds bytes >= 0x80 other than the two-byte
 * sequences C2 80..BF and C3 9F..BF / C3 97 (Latin-1 signs and LOWER-case letters) -- i.e. possibly an upper-case
 * non-ASCII letter, a rune whose lower-case form has another length, or invalid UTF-8.  The scan kernels notice high
 * bytes on their way; only such a batch pays one more pass over its text for this answer.
 * gft_finder_process_device checks it, lowers an unsafe batch with gft_to_lower_device's kernels and scans the lowered text
 * again; gft_to_lower_device does not touch it. */
int gft_last_nonascii(const gft_engine* e);
/* which scan kernel the built dictionary runs on: "scan5" (suffix-window kernel, one filter probe per two bytes: the
 * default wherever the long-term tables exist), "scan3" (stride-2 suffix-window kernel, any alphabet: the fallback) or
 * "dfa" (general two-tier DFA kernel: only when forced with GFT_SCAN_KERNEL); "scan2" / "scan4" (the earlier
 * suffix-window kernels) only in a library built with GFT_EXTRA_KERNELS (tools/, the opt-in cross-check job) */
const char* gft_scan_kernel(const gft_engine* e);
/* how this library was built: "gfx950 extra_kernels=0|1" (1: the cross-check kernels scan2 / scan4 are compiled in) */
const char* gft_build_info(void);

/* Caller-supplied matches (regex engine output, or the output of a foreign SubstringEngine), CSR per document.
 * `slot` is ABSOLUTE: n_terms + j for extra literal j, or a dictionary term id when a regex literal has the same
 * text as a keyword (both feed one map key in the reference, finder/finder.go:181-196).  Positions of one slot
 * must be ascending within a document (README.md:155). */
typedef struct gft_extra_matches {
    const uint64_t* off; /* n_docs + 1 */
    const uint32_t* slot;
    const uint32_t* pos;
} gft_extra_matches;

/* Finder.ProcessText over a batch: hit_bitmap[d * words + (i >> 5)] bit (i & 31) == expression i is true for
 * document d, words = ceil(n_exprs / 32).  `extra` may be NULL. */
int gft_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                const gft_extra_matches* extra, uint32_t* hit_bitmap);
/* Solve again over the documents of the LAST gft_process call on this engine (same n_docs), with other caller-supplied
 * matches: the scan results are still in the engine, only the solver kernel runs.  The finder's regex prefilter uses it:
 * first pass without regex hits, host regex engine on the candidate documents only, second pass with their hits. */
int gft_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap);
/* Device-resident variant of gft_process (all pointers are device pointers, bitmap written in HBM).  As for
 * gft_scan_device: d_text_blob needs no alignment, d_doc_off[0] may be non-zero, the bytes [0, d_doc_off[0]) and the 64 bytes
 * past d_doc_off[n_docs] must be readable (vector loads) and what they hold never changes the answer -- on every way a batch
 * gets its work units (gft_debug_last_unit_route), the deferred ones included, which tell the kernels nothing of the blob's end.
 * Documents of 4 GiB and more, and offsets that descend, are refused with GFT_E_INVALID. */
int gft_process_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                       uint32_t flags, const gft_extra_matches* d_extra, uint32_t* d_hit_bitmap);
/* The same, pipelined: _begin enqueues the batch (units -> scan -> solve -> the read-back of its control block) on the
 * engine's stream and returns WITHOUT waiting; _end completes the oldest batch begun and returns ITS status (and sets
 * gft_last_nonascii for it).  At most two batches are in flight, so a caller that begins batch i + 1 before it ends
 * batch i keeps the device busy while the host reads batch i's verdict and launches the next one -- what a step of 0.5 ms
 * (125 000 documents: one GPU's share of 1 M over 8) needs.  Where the text lies is as for gft_process_device: no alignment,
 * d_doc_off[0] may be non-zero, the bytes in front of the first document and the 64 bytes of slack are readable and never
 * change the answer; the two batches in flight may lie at different residues behind different lead bytes.  Inputs and the bitmap of a batch must stay untouched until its
 * _end has returned: a batch that outgrew the engine's unit table or match pool is run again there.  A batch that cannot be
 * deferred (caller-supplied matches, host-solved expressions, an engine's first batches, more documents than the unit
 * table holds) completes inside _begin; _end then only hands its status and its verdict back.  A batch is run again when
 * its scan overflowed the match pool IT was launched with, even if another batch has grown the pool since.  Single-device
 * handles.  Between _begin and _end no other entry point of the handle, except: _complete completes every batch in flight
 * in place (each keeps its status and verdict for its own _end), after which
 * the synchronous entry points (gft_process, gft_process_device) may run -- the finder repeats a batch that leaves ASCII
 * through them while a younger batch is in flight; gft_compact_device with total == NULL only enqueues (below).
 * gft_last_nonascii is the verdict of the batch whose _end, or whose synchronous call, returned last: _begin and _complete
 * do not touch it. */
int gft_process_device_begin(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                             uint32_t flags, const gft_extra_matches* d_extra, uint32_t* d_hit_bitmap);
int gft_process_device_end(gft_engine* e);
int gft_process_device_complete(gft_engine* e);

/* ---- Sparse results: the batch form of []ExpressionResult (finder/finder.go:25-29, 199-215) ------------------------------
 * A hit bitmap as CSR: the true expressions of document d are expr_idx[row_off[d] .. row_off[d + 1]), strictly ascending
 * (registration order, as solveExpressions emits them), row_off[n_docs] = their number over the batch; label[k] =
 * the label of expression expr_idx[k].  Labels are any uint32 per expression (the finder puts tag ids there); they belong to
 * a set of programs: labels is a host array of n == gft_n_exprs(e) entries, copied to the device; NULL / 0 clears; any
 * gft_set_programs clears them. */
int gft_set_expr_labels(gft_engine* e, const uint32_t* labels, uint32_t n);
/* Bitmap (device, layout as gft_process, gft_n_exprs(e) columns; bits at and above n_exprs in a row's last word are ignored)
 * -> CSR (device), built by three launches on the engine's stream (gft_profile_read: "compact_count", "compact_scan",
 * "compact_fill").  d_row_off: n_docs + 1 entries; d_expr_idx: cap entries (NULL with cap 0: count only); d_label: cap
 * entries or NULL (non-NULL without labels set: GFT_E_INVALID).  An entry whose position is >= cap is NOT written and nothing
 * is stored past cap entries, but d_row_off is always complete: GFT_OK is returned in both cases, the caller compares the
 * total with cap and calls again with larger buffers.  total (host) != NULL: the call waits for the stream and hands the
 * total back.  total == NULL: the call only enqueues and does not wait; the total is then in d_row_off[n_docs].  In that form
 * it may be called between gft_process_device_begin and _end: a pipelined caller compacts batch i, whose _end has returned,
 * while batch i + 1 is in flight.  n_docs == 0 and n_exprs == 0 are valid (d_row_off all zero).  Handles over several
 * devices (gft_engine_create_multi): GFT_E_UNSUPPORTED -- sparse gathers between devices are not built. */
int gft_compact_device(gft_engine* e, const uint32_t* d_hit_bitmap, uint64_t n_docs, uint64_t* d_row_off, uint32_t* d_expr_idx,
                       uint32_t* d_label, uint64_t cap, uint64_t* total);
/* gft_process with the CSR as its result (host buffers in; out's buffers are library-owned and stay valid until the next call
 * on the same engine; label == NULL when no labels are set).  When the rows are complete on the device -- no expression or
 * document the host solves -- they are compacted there and only the CSR comes down; otherwise, and on a handle over several
 * devices, the rows come down as for gft_process and are compacted on the host.  Both routes give the same arrays. */
typedef struct gft_sparse {
    uint64_t n_docs;
    uint64_t total;
    const uint64_t* row_off;   /* n_docs + 1 */
    const uint32_t* expr_idx;  /* total */
    const uint32_t* label;     /* total, or NULL */
} gft_sparse;
int gft_process_sparse(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                       const gft_extra_matches* extra, gft_sparse* out);
/* The compaction alone on the host, same contract (all pointers host; labels: n_exprs entries, needed when label != NULL).
 * No HIP device is needed: the finder uses this code for a batch whose bitmap was completed on the host, tests use it. */
int gft_debug_compact_host(const uint32_t* bitmap, uint64_t n_docs, uint32_t n_exprs, const uint32_t* labels, uint64_t* row_off,
                           uint32_t* expr_idx, uint32_t* label, uint64_t cap, uint64_t* total);

/* ---- strings.ToLower over a batch on the device (finder/finder.go:140-142; csrc/gft_tolower.hip) -------------------------
 * (d_text_blob, d_doc_off [n_docs + 1]) -> (d_out, d_out_off [n_docs + 1]): byte for byte what gft_to_lower gives for every
 * document, concatenated, d_out_off[0] = 0.  Go's decoder: an invalid byte -- a continuation byte out of place, C0 / C1,
 * F5..FF, an overlong form, a surrogate, F4 90.., a lead byte that ITS DOCUMENT does not continue -- becomes one U+FFFD; the
 * bytes of a neighbouring document never complete a rune.  Lengths change (U+0130, U+212A shrink, U+023A, U+023E grow, an
 * invalid byte becomes three): the output has at most three times the input's bytes.  Three passes on the engine's stream
 * (gft_profile_read: "lower_count", "lower_scan", "lower_write"); the contract mirrors gft_compact_device: d_out_off is always
 * complete, a byte whose output position is >= cap is NOT written and nothing is stored at or past d_out + cap, GFT_OK is
 * returned in both cases and *total (host, nullable) receives the lowered size -- the caller compares it with cap and calls
 * again.  d_out == NULL with cap == 0 counts only.  The call waits for the stream.  d_text_blob must be readable for 64 bytes
 * past d_doc_off[n_docs], as for the scans; the output (d_out, d_out_off) may not overlap the input: GFT_E_INVALID, as for
 * offsets that descend and for a document, or the lower-case form of one, of 4 GiB or more.  n_docs == 0 is valid.  Handles
 * over several devices: GFT_E_UNSUPPORTED.  Between gft_process_device_begin and _end only after _complete.  Needs no
 * dictionary, leaves gft_last_nonascii alone, and the handle stays usable after any error. */
int gft_to_lower_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_out,
                        uint64_t cap, uint64_t* d_out_off, uint64_t* total);
/* The same on the host, no HIP device needed (tests): the lower-case form of ONE code point looked up in the two-level table
 * the kernels read (derived from the pairs behind gft_to_lower when first used) ... */
uint32_t gft_debug_lower_rune(uint32_t cp);
/* ... and gft_to_lower_device's count / prefix / write walk, unit by unit and 16-byte piece by piece through the source the
 * kernels are compiled from (csrc/gft_tolower_piece.hpp).  All pointers host; same contract and refusals (the 64 bytes of
 * slack are not asked for here). */
int gft_debug_emulate_to_lower(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* out, uint64_t cap,
                               uint64_t* out_off, uint64_t* total);

/* ---- A resident blob cut into line documents on the device (csrc/gft_split.hip) -------------------------------------------
 * (d_blob, len) -> d_doc_off [n + 1]: the offset array every batch entry point takes, made where the text lies.  Two modes: */
enum gft_split_mode {
    GFT_SPLIT_AFTER_NL = 0,   /* Go's strings.SplitAfter(blob, "\n") without a final empty piece: a document starts at 0 and at
                               * every p + 1 with blob[p] == '\n' and p + 1 < len; a '\n' stays with the document it ends;
                               * len == 0 gives no document */
    GFT_SPLIT_JSON_LINES = 1  /* JSON Lines: a line begins at 0 and behind every '\n' and is blank when it holds nothing but the
                               * JSON whitespace bytes 20 09 0A 0D.  Document 0 starts at 0, document i >= 1 where the i-th
                               * non-blank line (counted from 0) starts: blank lines, '\r', indentation and the newline travel
                               * with the document in front of them, those in front of the first non-blank line with document
                               * 0.  A blob of whitespace gives no document.  Every document is one line's JSON value with
                               * whitespace round it -- what the walker of the group finder's JSON calls and its host reader
                               * accept unchanged */
};
/* d_doc_off[0..n] is written with d_doc_off[0] = 0 and d_doc_off[n] = len; n == 0 writes d_doc_off[0] = 0 only.  Three launches
 * on the engine's stream (gft_profile_read: "split_count", "split_scan", "split_write"); the cap protocol is gft_compact_device's:
 * cap counts entries of d_doc_off, an entry whose index is >= cap is NOT written and nothing is stored at or past
 * d_doc_off + cap, GFT_OK is returned in both cases and *n_docs (host) receives n -- the caller compares n + 1 with cap and
 * calls again.  d_doc_off == NULL with cap == 0 counts only.  The call waits for the stream.  d_blob must be readable for 64
 * bytes past len, as for the scans (what those bytes hold never changes the answer), and needs no alignment.  Offsets and counts
 * are 64-bit throughout: a document of 4 GiB or more is not refused here -- the calls that take the result refuse it.
 * GFT_E_INVALID: an unknown mode, an output that overlaps the input.  Handles over several devices: GFT_E_UNSUPPORTED.  Between
 * gft_process_device_begin and _end only after _complete.  Needs no dictionary, leaves gft_last_nonascii alone, and the handle
 * stays usable after any error. */
int gft_split_lines_device(gft_engine* e, const uint8_t* d_blob, uint64_t len, uint32_t mode, uint64_t* d_doc_off, uint64_t cap,
                           uint64_t* n_docs);
/* The same on the host, no HIP device needed: the kernels' walk tile by tile through the source they are compiled from
 * (csrc/gft_split_piece.hpp), with the same carry resolution.  All pointers host; same contract; the 64 bytes of slack are not
 * asked for here.  It is also what gft_group_process_json_lines splits with when the finder does not take the device route. */
int gft_debug_split_lines(const uint8_t* blob, uint64_t len, uint32_t mode, uint64_t* doc_off, uint64_t cap, uint64_t* n_docs);
/* where that walk's borders are: the bytes a wave owns (a tile), and the tiles one trip of the carry pass resolves */
void gft_debug_split_shape(uint32_t* tile_bytes, uint32_t* tiles_per_carry_trip);

/* ---- The documents that matched, gathered into one blob on the device (csrc/gft_select.hip) -------------------------------
 * (d_text_blob, d_doc_off [n_docs + 1], hit rows, a column mask) -> the selected documents' bytes back to back in input order,
 * their offsets and their input indices: the filter step behind gft_process_device / gft_group_process_jsons_device, made where
 * the text lies.  A document is selected by its row under one of three modes: */
enum gft_select_mode {
    GFT_SELECT_ANY = 0,   /* (row & want) != 0 */
    GFT_SELECT_ALL = 1,   /* (row & want) == want  -- an empty want selects every document */
    GFT_SELECT_NONE = 2   /* (row & want) == 0    -- the complement of ANY */
};
/* d_bitmap [n_docs][W], W = ceil(n_cols / 32), layout of gft_process; n_cols is explicit so that finder rows (gft_n_exprs) and
 * the group finder's rule rows (gft_group_n_rule_exprs) go through one call.  Bits at and above n_cols in a row's last word are
 * ignored, whatever they hold.  want: HOST memory, W words, copied by the call; NULL = every column; its bits at and above
 * n_cols are ignored too.  n_cols == 0 is valid and needs no d_bitmap: ANY selects nothing, ALL and NONE every document.
 * d_also (nullable) [n_docs] bytes: non-zero = the document is selected whatever its row says (the status bytes of
 * gft_group_process_jsons_device: a document the device did not decide is never silently dropped; d_doc_idx tells which it was).
 * With m selected documents of `total` bytes: d_out receives them back to back in input order, d_out_off[0..m] where each
 * starts (d_out_off[0] = 0, d_out_off[m] = total), d_doc_idx[k] the input index of output document k.
 * Cap protocol of gft_compact_device: cap_bytes counts bytes of d_out, cap_docs entries of d_doc_idx, and d_out_off has
 * cap_docs + 1 entries.  A byte whose output position is >= cap_bytes, an index entry >= cap_docs and an offset entry > cap_docs
 * are NOT written; nothing at all is stored at or past d_out + min(total, cap_bytes) -- byte-exactly, no rounding up to a store
 * width --; GFT_OK is returned in both cases and *n_selected = m, *total_bytes = total (host, nullable) are always handed back
 * -- the caller compares them with the caps and calls again.  d_out == NULL with cap_bytes == 0, and d_out_off == d_doc_idx ==
 * NULL with cap_docs == 0, count only (a d_out_off that is not NULL always receives entry 0).  n_docs == 0 is valid.
 * Four launches on the engine's stream (gft_profile_read: "select_mark", "select_scan", "select_place", "select_copy"); the call
 * waits for the stream.  d_text_blob must be readable for 64 bytes past d_doc_off[n_docs], as for the scans (what those bytes
 * hold never changes the answer), and needs no alignment; d_out needs none either.
 * GFT_E_INVALID: an unknown mode; a cap without its array; offsets that descend or a document of 4 GiB or more (selected or
 * not; found on the device as gft_to_lower_device finds them); an output that overlaps the text, the offsets, the bitmap, d_also
 * or another output.  Handles over several devices: GFT_E_UNSUPPORTED.  GFT_E_NOMEM: no room for the work buffers (24 bytes a
 * document and 16 a selected one).  Between gft_process_device_begin and _end only after _complete.  Needs no dictionary and no programs, leaves
 * gft_last_nonascii alone, and the handle stays usable after any error. */
int gft_select_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap,
                           uint32_t n_cols, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint8_t* d_out, uint64_t cap_bytes,
                           uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes);
/* The same on the host, no HIP device needed: the kernels' walk tile by tile through the source they are compiled from
 * (csrc/gft_select_piece.hpp).  All pointers host; same contract and refusals; only blob[doc_off[0], doc_off[n_docs]) is read:
 * the 64 bytes of slack are not asked for here.  It is also what a finder selects with when a batch's rows were completed on
 * the host. */
int gft_debug_select_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                          const uint32_t* want, uint32_t mode, const uint8_t* also, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                          uint64_t* doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes);
/* where that walk's borders are: the bytes of the output a lane stores at once (a chunk, aligned to the output address), a
 * wave's trip, and the bytes a wave owns (a tile) */
void gft_debug_select_shape(uint32_t* chunk_bytes, uint32_t* trip_bytes, uint32_t* tile_bytes);

/* ---- Context lines: the selected documents and the ones round them, on the device (csrc/gft_context.hip) -----------------
 * grep -A / -B / -C over a resident batch whose documents are lines.  d_text_blob, d_doc_off, d_bitmap, n_cols, want (HOST), mode
 * and d_also are those of gft_select_docs_device, and a document is SELECTED when that call would select it.  Document d is KEPT
 * when some selected h satisfies d - after <= h <= d + before -- saturating: before and after may be 2^64 - 1 -- and no fence lies
 * between h and d.  d_fence (nullable) [n_docs] bytes: a non-zero byte at f forbids context from crossing between f - 1 and f (a
 * file border of a concatenated log, a bucket border of a routed blob): h and d are separated when a fence index lies in
 * (min(h, d), max(h, d)].  d_fence[0] changes nothing.
 * With m kept documents of `total` bytes: d_out, d_out_off [0..m] and d_doc_idx [m] are the select's outputs for the kept
 * documents, in input order.  d_kind[r] = 1 when kept document r is itself selected, 0 when it is context only (grep's ':' and
 * '-').  A group is a maximal run of kept documents with consecutive input indices and no fence inside (grep prints "--" between
 * groups): d_group_off[g] is the rank r at which group g begins, d_group_off[n_groups] = m.
 * Cap protocol of gft_select_docs_device: cap_bytes counts bytes of d_out (byte-exact); cap_docs entries of d_doc_idx and d_kind,
 * d_out_off has cap_docs + 1; d_group_off has cap_groups + 1 and nothing is stored at d_group_off[> cap_groups].  *n_kept,
 * *n_hits (the selected documents), *n_groups and *total_bytes (host, nullable) are always complete.  All device outputs NULL
 * with all caps 0 counts only; an offset array that is not NULL always receives entry 0.  n_docs == 0 is valid.
 * With before == after == 0 and no fence, d_out, d_out_off and d_doc_idx are those of gft_select_docs_device, d_kind is all 1 and
 * the groups are the maximal runs of selected documents.
 * Launches on the engine's stream (gft_profile_read: "context_mark", "context_reach", "context_carry", "context_decide",
 * "context_scan", "context_place", "context_copy"); the call waits for the stream.  Slack and alignment as for the select.
 * GFT_E_INVALID: a null argument; a cap without its array; an unknown mode; offsets that descend or a document of 4 GiB or more;
 * an output that overlaps an input or another output.  Handles over several devices: GFT_E_UNSUPPORTED.  GFT_E_NOMEM: no room for
 * the work buffers (36 bytes a document, a few words per 64 documents and 16 bytes a kept one).  Between gft_process_device_begin
 * and _end only after _complete.  Needs no dictionary and no programs, leaves gft_last_nonascii alone, and the handle stays usable
 * after any error. */
int gft_context_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap,
                            uint32_t n_cols, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint64_t before, uint64_t after,
                            const uint8_t* d_fence, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint8_t* d_kind,
                            uint64_t cap_docs, uint64_t* d_group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups,
                            uint64_t* total_bytes);
/* The same on the host, no HIP device needed: the kernels' walk tile by tile through the source they are compiled from
 * (csrc/gft_context_piece.hpp).  All pointers host; same contract and refusals; only blob[doc_off[0], doc_off[n_docs]) is read.
 * It is also what a finder takes when a batch's rows were completed on the host. */
int gft_debug_context_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                           const uint32_t* want, uint32_t mode, const uint8_t* also, uint64_t before, uint64_t after, const uint8_t* fence,
                           uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint8_t* kind, uint64_t cap_docs,
                           uint64_t* group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups, uint64_t* total_bytes);
/* where that walk's borders are: the documents a wave owns (a tile), the tiles of a carry block, and the carry blocks one trip
 * of the spine pass resolves */
void gft_debug_context_shape(uint32_t* tile_docs, uint32_t* carry_block_tiles, uint32_t* spine_trip_blocks);

/* ---- Documents routed to per-bucket runs of one blob on the device (csrc/gft_route.hip) ----------------------------------
 * The K-way form of the select above: n_buckets column masks instead of one, and the output is ONE blob in which every bucket is
 * a contiguous run -- a stable counting sort of (document, bucket) entries in front of the select's copy kernel. */
enum gft_route_mode {
    GFT_ROUTE_FIRST = 0,  /* a routing table: a document goes to the lowest-numbered bucket whose mask it hits, only there */
    GFT_ROUTE_EVERY = 1   /* a document goes to every bucket whose mask it hits: one entry, and one copy of its bytes, per bucket */
};
#define GFT_ROUTE_REST 1u        /* flags: one more bucket, numbered n_buckets, for the documents that hit no mask */
#define GFT_ROUTE_MAX_BUCKETS 64 /* n_buckets plus the rest bucket */
/* d_text_blob, d_doc_off, d_bitmap and n_cols as for gft_select_docs_device (64 bytes of slack behind the text, no alignment,
 * d_doc_off[0] may be non-zero; finder rows and the group finder's rule rows go through the one call).  masks: HOST memory,
 * n_buckets x W words, W = ceil(n_cols / 32), copied by the call.  Document d hits bucket k when (row[d] & masks[k]) != 0, both
 * cut to n_cols: bits at and above n_cols are ignored in rows and in masks, whatever they hold.  n_cols == 0 needs no d_bitmap
 * and no masks: no document then hits any mask.  n_buckets == 0 is valid.
 * B = n_buckets + (flags & GFT_ROUTE_REST ? 1 : 0) buckets; B > GFT_ROUTE_MAX_BUCKETS: GFT_E_UNSUPPORTED.  Without GFT_ROUTE_REST
 * a document that hits no mask produces no entry.  d_also (nullable) [n_docs] bytes: non-zero = the document goes to the rest
 * bucket and nowhere else, in both modes (the status bytes of gft_group_process_jsons_device: the device did not decide the
 * document, its row means nothing and it must not be dropped); d_also without GFT_ROUTE_REST: GFT_E_INVALID.
 * The result is a list of m entries (document, bucket) ordered by bucket first and by input index inside a bucket (stable):
 * d_out holds the entries' documents back to back in that order, d_out_off[0..m] where each starts (d_out_off[0] = 0),
 * d_doc_idx[r] the input index of entry r.  bucket_doc, bucket_byte: HOST arrays of B + 1 entries (nullable): bucket b's entries
 * are [bucket_doc[b], bucket_doc[b + 1]) and its bytes d_out[bucket_byte[b] .. bucket_byte[b + 1]); bucket_doc[B] = m and
 * bucket_byte[B] = the total.  When given they are always complete, whatever the caps: they take the place of the select's
 * n_selected and total_bytes.  Empty documents are entries like any other.
 * Cap protocol of gft_select_docs_device: cap_bytes counts bytes of d_out, cap_docs entries; nothing is stored at or past
 * d_out + min(total, cap_bytes) -- byte-exactly --, at d_doc_idx[>= cap_docs] or at d_out_off[> cap_docs]; GFT_OK in both cases.
 * All outputs NULL with both caps 0 counts only (a tag histogram: no bitmap crosses the link).  n_docs == 0 is valid:
 * d_out_off[0] = 0 if given, the host arrays all zero.  The call waits for the stream; it synchronises with the host once in
 * the middle (the entry count, the bucket borders and the total come back together).
 * Launches on the engine's stream (gft_profile_read: "route_mark", "route_count", "route_scan", "route_place", "route_copy").
 * GFT_E_INVALID: an unknown mode; unknown flag bits; a cap without its array; offsets that descend or a document of 4 GiB or more
 * (found on the device); an output that overlaps an input or another output.  Handles over several devices: GFT_E_UNSUPPORTED.
 * GFT_E_NOMEM: no room for the work buffers -- 12 bytes a document (member word, length), 12 bytes a (bucket, tile of 64
 * documents) (count, base) and 8 a tile (its bytes), 20 bytes an entry (length, output offset, source offset), the masks and the
 * scans' partials.  Between gft_process_device_begin and _end only after _complete.  Needs no dictionary and no programs, leaves
 * gft_last_nonascii alone, and the handle stays usable after any error. */
int gft_route_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                          const uint32_t* d_bitmap, uint32_t n_cols,
                          const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* d_also,
                          uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs,
                          uint64_t* bucket_doc, uint64_t* bucket_byte);
/* The same on the host, no HIP device needed: the kernels' walk tile by tile through the source they are compiled from
 * (csrc/gft_route_piece.hpp, and the select's copy walk).  All pointers host; same contract and refusals; only
 * blob[doc_off[0], doc_off[n_docs]) is read.  It is also what a finder routes with when it does not take the device route. */
int gft_debug_route_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                         const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* also,
                         uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint64_t cap_docs,
                         uint64_t* bucket_doc, uint64_t* bucket_byte);
/* where that walk's borders are: the documents a counting tile (a wave) holds */
void gft_debug_route_shape(uint32_t* tile_docs);

/* ---- Hit spans and redaction on the device: where the expressions matched (csrc/gft_spans.hip) ------------------------------
 * The step behind gft_process_device, the select and the route: for a resident batch and its hit rows, the byte spans of the
 * keyword occurrences that belong to a true, wanted expression -- and the overwrite of exactly those bytes with a mask byte.
 * Witness terms: P(i), the witness terms of expression i, are the dictionary slots (slot < gft_n_terms) of the GFT_OP_UNIT words
 * of its public postfix program that lie outside the operand of every GFT_OP_NOT.  A unit under a NOT is no witness, whatever
 * the nesting -- one under two NOTs is not either: a NOT removes the units below it and nothing restores them.  INORD changes
 * nothing.  Extra slots (>= n_terms: regex literals, caller-supplied matches) are never witnesses, the library has no length for
 * them; an extra literal with the text of a keyword shares the keyword's term id and counts through it.  A slot that occurs twice
 * in an expression is listed once.  This is the rule "highlight every query term of a matching query": in a true
 * ("a" and "b") or "c" an occurrence of a is kept even if b is absent -- no minimal witness (which branch of an OR fired) is
 * attempted.
 * Kept matches: a match (document d, term t, pos) of the canonical CSR -- what gft_scan_device gives for the batch -- is kept
 * when some expression i with t in P(i) has its bit set in `want` and in row r(d) of the hit bitmap (layout of gft_process,
 * gft_n_exprs columns).  Bits at and above n_exprs are ignored in rows and in want, whatever they hold.  want: HOST memory,
 * W = ceil(n_exprs / 32) words, copied by the call; NULL = every expression.  r(d) = d, or d_row_idx[d] with d_row_idx (nullable,
 * uint64 [n_docs]): the blob a select or a route produced is explained against the bitmap of the batch it came from -- their
 * d_doc_idx output is exactly this array; repeated indices (a document routed to two buckets) are valid.  Every index must name a
 * row of d_hit_bitmap: the call cannot know how many it has.
 * Spans: len = the term's byte length; start = pos on a GFT_POS_START engine, pos + 1 - len on a GFT_POS_END engine; both uint32,
 * relative to the document's first byte.  term = the term id.  The kept matches of a document stay in the order gft_scan_device
 * gives them (the compaction is stable): the spans of document d are [d_span_off[d], d_span_off[d + 1]), d_span_off[0] = 0,
 * d_span_off[n_docs] = the total.
 * The call runs the scan with positions and the canonical CSR, as gft_scan_device does, under its placement contract: no
 * alignment, d_doc_off[0] may be non-zero, 64 readable bytes of slack behind d_doc_off[n_docs], and neither the slack nor the lead
 * bytes ever change the answer.  Behind the scan three launches on the engine's stream (gft_profile_read: "span_mark",
 * "span_scan", "span_place"); the call waits for the stream.  It counts as a scan: it publishes gft_last_nonascii for the batch
 * and leaves the engine's scan state as gft_scan_device leaves it.  flags: GFT_FOLD_ASCII; GFT_SCAN_UNIQUE and GFT_POS_RUNES:
 * GFT_E_INVALID.
 * Cap protocol of gft_compact_device: cap counts span entries; an entry at or past cap is NOT written and nothing is stored at or
 * past any array + cap; d_span_off (n_docs + 1 entries, nullable, always complete when given) is not capped; all span arrays NULL
 * with cap == 0 counts only; GFT_OK in both cases and *total (host, nullable) is always handed back -- the caller compares it with
 * cap and calls again.  d_span_len and d_span_term may each be NULL on their own.
 * Needs a dictionary and programs (GFT_E_NOT_BUILT).  Handles over several devices: GFT_E_UNSUPPORTED.  Between
 * gft_process_device_begin and _end only after _complete.  n_docs == 0 and n_exprs == 0 are valid and give no span.  An output
 * that overlaps the text, the offsets, the bitmap (its first n_docs rows; with d_row_idx its first row), d_row_idx or another
 * output: GFT_E_INVALID.  GFT_E_NOMEM: no room for the work buffers (12 bytes a match).  The handle stays usable after any error.
 * Cost note: a term that stands in thousands of expressions makes the walk of one match that long when none of them is true and
 * wanted (DESIGN.md 7 #2k). */
int gft_hit_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                         const uint32_t* d_hit_bitmap, const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off,
                         uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap, uint64_t* total);
/* In place: byte d_doc_off[d] + start + k for k < len of every span (d_span_off [n_docs + 1], spans [d_span_off[0],
 * d_span_off[n_docs]) of d_span_start / d_span_len) becomes mask_byte; every other byte of the buffer keeps its value,
 * byte-exactly -- the lead bytes, the slack, the neighbours of a span's first and last byte: the fill stores single bytes.  Spans
 * may overlap, nest and repeat.  mask_byte > 255: GFT_E_INVALID.  A span that reaches past its document's end is found on the
 * device, before the fill, and refused with GFT_E_INVALID: nothing at all is written then, inside the documents or outside.
 * gft_profile_read: "redact_fill" (the check pass that resolves every span's address and the fill pass run under that one name).
 * Masking whole keyword occurrences byte by byte keeps valid UTF-8 valid when the mask is ASCII, and the result has the same
 * length: the offsets stay good.  Needs no dictionary and no programs, leaves gft_last_nonascii alone; handles over several
 * devices: GFT_E_UNSUPPORTED; between gft_process_device_begin and _end only after _complete; GFT_E_NOMEM: no room for the work
 * buffer (8 bytes a span); n_docs == 0 and no spans are valid; the handle stays usable after any error. */
int gft_redact_spans_device(gft_engine* e, uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                            const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t mask_byte);
/* The host forms, no HIP device needed, same contracts, all pointers host.  The witness table of a set of programs as the
 * term -> expressions CSR the kernels read (csrc/witness_terms.cpp): off [n_terms + 1] (nullable, always complete), expr (cap
 * entries; NULL with cap 0 counts only) ascending per term, *needed = their number.  GFT_E_INVALID: a program that is no postfix
 * expression, a slot >= n_slots. */
int gft_debug_witness_terms(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_terms, uint32_t n_slots,
                            uint64_t* off, uint32_t* expr, uint64_t cap, uint64_t* needed);
/* gft_hit_spans_device behind its scan: the kernels' walk, match tile by match tile through the source they are compiled from
 * (csrc/gft_spans_piece.hpp), over a match CSR (match_off[0] = 0), the terms' lengths and a witness table. */
int gft_debug_hit_spans(const uint64_t* match_off, const uint32_t* term_id, const uint32_t* pos, uint64_t n_docs, const uint32_t* term_len,
                        uint32_t pos_end, const uint64_t* wit_off, const uint32_t* wit_expr, const uint32_t* bitmap, uint32_t n_exprs,
                        const uint64_t* row_idx, const uint32_t* want, uint64_t* span_off, uint32_t* span_start, uint32_t* span_len,
                        uint32_t* span_term, uint64_t cap, uint64_t* total);
/* gft_redact_spans_device: the check and the fill's walk, span tile by span tile and lane by lane through the same header. */
int gft_debug_redact_spans(uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                           const uint32_t* span_len, uint32_t mask_byte);
/* where those walks' borders are: the matches a workgroup of the mark pass takes per step, the spans a wave of the fill owns */
void gft_debug_spans_shape(uint32_t* tile_matches, uint32_t* tile_spans);

/* ---- Spans of a lowered batch mapped back to the source text (csrc/gft_lowermap.hip) ---------------------------------------------
 * strings.ToLower changes lengths (U+0130 and U+212A shrink, U+023A grows, an invalid byte becomes the three bytes of U+FFFD), so
 * the spans gft_hit_spans_device gives for the LOWERED form of a batch (gft_to_lower_device) do not index the text the caller
 * holds.  This call rewrites them, in place, to positions in the SOURCE batch; it needs neither the lowered text nor its offsets:
 * the map is a function of the source alone.
 * Go's decoder cuts a document S into runes: a valid sequence of 1..4 bytes, or ONE byte that decodes to U+FFFD.  Rune i takes the
 * source bytes [a_i, a_i + sl_i) and the lowered bytes [b_i, b_i + ll_i), ll_i >= 1; B = the lowered length.  A lowered span
 * (start, len) with len >= 1 maps to [a_p, a_q + sl_q): p the rune whose lowered bytes hold byte start, q the one that holds byte
 * start + len - 1 -- a span that cuts a lowered rune covers the whole source rune.  len == 0 maps to (a_p, 0), and at start == B to
 * (the length of S, 0).  So: source spans begin and end on the source's rune cuts -- masking them with an ASCII byte keeps valid
 * UTF-8 valid; a text masked through them has the caller's length and the caller's offsets; and on a fold-safe document the map
 * is the identity.
 * d_text_blob / d_doc_off: the source batch under the scans' placement contract (no alignment, d_doc_off[0] may be non-zero, 64
 * readable bytes of slack; neither the slack nor the lead bytes ever change the answer; documents are judged one by one, as
 * gft_to_lower_device judges them).  d_span_off [n_docs + 1] / d_span_start / d_span_len: what gft_hit_spans_device wrote for the
 * lowered form of this batch -- the spans [d_span_off[0], d_span_off[n_docs]).  A span with start + len > B is found on the device,
 * before anything is written, and refused with GFT_E_INVALID: nothing at all is written then.
 * Two parts on the engine's stream (gft_profile_read): "lowermap_table" -- gft_to_lower_device's count pass and prefix sum, then
 * its walk once more, storing where every 16-byte piece's output begins in its document's lowered form: 4 bytes per 16 source
 * bytes -- and "lowermap_spans" -- a lane a span: a check pass (the span's document, two binary searches, the rune inside the piece
 * found) and a write pass.  The call waits for the stream.  Needs no dictionary, leaves gft_last_nonascii alone.  Handles over
 * several devices: GFT_E_UNSUPPORTED.  Between gft_process_device_begin and _end only after _complete.  n_docs == 0 and no spans
 * are valid.  GFT_E_INVALID: a span array that overlaps the text, the offsets or the other span array; offsets that descend; a
 * document, or the lower-case form of one, of 4 GiB or more.  GFT_E_NOMEM: no room for the work buffers (4 bytes per 16 of text,
 * 8 bytes a span).  The handle stays usable after any error. */
int gft_map_spans_to_source_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                   const uint64_t* d_span_off, uint32_t* d_span_start, uint32_t* d_span_len);
/* The host form, no HIP device needed, same contract, all pointers host (the 64 bytes of slack are not asked for here): the table
 * unit by unit and piece by piece, the map span by span, through the source the kernels are compiled from
 * (csrc/gft_tolower_piece.hpp, csrc/gft_lowermap_piece.hpp). */
int gft_debug_map_spans_to_source(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                  uint32_t* span_start, uint32_t* span_len);
/* where that walk's borders are: the bytes of a piece, of a wave's trip and of a work unit at most; the spans of a wave's tile */
void gft_debug_lowermap_shape(uint32_t* piece_bytes, uint32_t* trip_bytes, uint32_t* unit_bytes, uint32_t* tile_spans);

/* ---- Excerpts on the device: the text around the hits, cut and gathered (csrc/gft_excerpt.hip) -------------------------------
 * The last step of split -> process -> (select | route) -> spans -> (map) -> excerpt: for a resident batch and its hit spans, the
 * windows of text around the spans, merged where they meet, back to back in one blob -- with the index arrays that tie every
 * excerpt to its document and every span to its excerpt.  A view of the text the caller gave: no scan, no dictionary.
 * Input: the batch under the scans' placement contract (no alignment, d_doc_off[0] may be non-zero, 64 readable bytes of slack
 * behind d_doc_off[n_docs]; neither the lead bytes nor the slack ever change the answer) and the span CSR gft_hit_spans_device
 * wrote for it, or gft_map_spans_to_source_device rewrote for its source: the spans [d_span_off[0], d_span_off[n_docs]) of
 * d_span_start / d_span_len.
 * Window: of span (start, len) in document d of L bytes, [max(0, start - before), min(L, start + len + after)), in 64 bits:
 * before = after = 0xFFFFFFFF gives the whole document.  With GFT_EXCERPT_RUNES in flags a window is widened so that it cuts no
 * UTF-8 sequence: its start moves back while the byte at the start is a continuation byte 10xxxxxx, its end forward while the
 * byte at the end is one; each at most three steps, neither past the document's first byte or its end.  Only bytes of the
 * document itself are consulted -- never the lead, the slack or a neighbouring document.
 * Merge: the excerpts of a document are the connected components of the union of its windows; windows that overlap or touch
 * (a.end == b.start) are one excerpt, a gap of one byte separates two.  Excerpts never cross a document border, even where two
 * documents' windows touch in the blob.  A window of no bytes (a len == 0 span with before = after = 0, a span of an empty
 * document) that touches no other is an excerpt of no bytes.
 * Span order: within a document the spans' ends start + len must not descend -- the scan's canonical order (end ascending, length
 * descending) guarantees it and the monotone source map keeps it.  A batch that breaks the order, or a span with start + len > L,
 * is found on the device before anything is written: GFT_E_INVALID, and nothing at all is written.  Under this order the excerpts
 * are runs of consecutive spans, which is why the outputs index the caller's own span arrays.
 * Outputs, device memory, each nullable on its own: d_out, the excerpts back to back in span order (= document order); d_exc_off
 * [n_exc + 1], usable as the doc_off of d_out; d_exc_doc, the document of each excerpt; d_exc_start, its first byte relative to
 * its document; d_exc_span_off [n_exc + 1]: excerpt k holds the spans [d_exc_span_off[k], d_exc_span_off[k + 1]) of the caller's
 * span arrays; d_span_rel, parallel to d_span_start (the entries [d_span_off[0], d_span_off[n_docs]) are written): each span's
 * start relative to its excerpt; d_doc_exc_off [n_docs + 1], the documents' CSR over the excerpts.  (d_out, d_exc_off, n_exc,
 * d_exc_span_off, d_span_rel, d_span_len) is a valid argument list of gft_redact_spans_device: masking inside the excerpts needs
 * no further call.
 * Cap protocol of gft_compact_device with two caps: cap_exc counts excerpt entries (d_exc_off and d_exc_span_off have cap_exc + 1,
 * d_exc_doc and d_exc_start cap_exc), cap_bytes bytes of d_out; nothing is stored at or past any array + cap; an excerpt that
 * cap_bytes cuts is written up to the cap, and d_exc_off keeps the uncut offsets.  The d_exc_span_off entries below the cap -- the
 * last of them, d_exc_span_off[cap_exc], too -- are indexes into the caller's span arrays like all the others: they count from the
 * arrays' first entry, not from d_span_off[0].  d_span_rel and d_doc_exc_off are sized by the
 * input, are never capped and are complete when given.  All outputs NULL with both caps 0 counts only; GFT_OK either way, and
 * *n_exc / *total_bytes (host, nullable) are always handed back.
 * Launches on the engine's stream (gft_profile_read): "excerpt_window" (a lane a span: its document by a binary search, the
 * window, the snap, the checks), "excerpt_smin" (the suffix minimum of the window starts over the whole batch: tile minima, one
 * workgroup's carry trips, the tiles' scans; heads marked), "excerpt_scan" (two prefix sums), "excerpt_place", "excerpt_copy" (the
 * select's copy kernel: a lane a 16-byte chunk of the output).  The call waits for the stream.
 * Needs no dictionary and no programs; leaves gft_last_nonascii alone.  Handles over several devices: GFT_E_UNSUPPORTED.  Between
 * gft_process_device_begin and _end only after _complete.  n_docs == 0, no spans and len == 0 spans are valid.  GFT_E_INVALID:
 * unknown flag bits; an output that overlaps an input or another output; document or span offsets that descend; a document of
 * 4 GiB or more.  GFT_E_NOMEM: no room for the work buffers (56 bytes a span, 16 an excerpt).  The handle stays usable after any
 * error. */
#define GFT_EXCERPT_RUNES 1u
int gft_excerpt_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                             const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t before,
                             uint32_t after, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc,
                             uint32_t* d_exc_start, uint64_t* d_exc_span_off, uint64_t cap_exc, uint32_t* d_span_rel,
                             uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes);
/* The host form, no HIP device needed, same contract, all pointers host (the 64 bytes of slack are not asked for here): the
 * passes tile by tile, carry trip by carry trip and lane by lane through the source the kernels are compiled from
 * (csrc/gft_excerpt_piece.hpp); the copy is a memcpy per excerpt. */
int gft_debug_excerpt_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                            const uint32_t* span_start, const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags,
                            uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start,
                            uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc,
                            uint64_t* total_bytes);
/* where that walk's borders are: the spans of a tile of the suffix-minimum scan, the tiles of one carry trip */
void gft_debug_excerpt_shape(uint32_t* tile_spans, uint32_t* trip_tiles);

/* Excerpts snapped to word or line borders: gft_excerpt_spans_device with two more flag bits and `reach`, the most bytes a snap
 * may move an edge (at most GFT_EXCERPT_REACH_MAX: a lane walks its edges byte by byte, rune by rune).  With neither bit, or with
 * reach == 0, the call is gft_excerpt_spans_device bit for bit and launches the same kernels.
 * The window [lo, hi) of a span in its document D of L bytes is the one above -- clipped, then rune-snapped when
 * GFT_EXCERPT_RUNES or GFT_EXCERPT_WORDS is set: the word snap implies the rune snap --, and then grows by ONE of two snaps.
 * GFT_EXCERPT_WORDS.  A position p, 0 < p < L, CUTS A WORD iff word(utf8.DecodeLastRune(D[:p])) and word(utf8.DecodeRune(D[p:])),
 * with the word class and the two strict decoders of gft_filter_word_matches_device: RuneError is no word rune, and nothing
 * outside D is read -- not the lead, the slack, a neighbouring document or the other half of a rune a document border cuts.
 * Start: p = lo; while p cuts a word, with r the size of the rune that ends at p: if lo - (p - r) > reach the start STAYS lo (the
 * word is longer than the reach: given up, not cut `reach` bytes further out), else p -= r.  End: p = hi; while p cuts a word,
 * with r the size of the rune at p: if (p + r) - hi > reach the end stays hi, else p += r.
 * GFT_EXCERPT_LINES.  No decoding, and no rune snap unless GFT_EXCERPT_RUNES asks for it.  Start: p = lo; while p > 0 and
 * D[p - 1] != '\n': if lo - (p - 1) > reach the start stays lo, else p--.  End: p = hi; while p < L and D[p] != '\n': if
 * (p + 1) - hi > reach the end stays hi, else p++.  The newline itself lies outside the window, so hits on two adjacent lines are
 * two excerpts; '\r' is a byte like any other.  before = after = 0 gives the lines the hits stand in: grep's output inside every
 * document.
 * Both snaps only grow a window (a span stays inside its own), are monotone in the edge they start from, stay inside [0, L] and
 * move no edge by more than reach.  Everything else -- merge, span order, outputs, cap protocol, profile names, work buffers, the
 * refusals -- is gft_excerpt_spans_device's; GFT_EXCERPT_WORDS uploads the word class table on a handle's first such call.
 * GFT_E_INVALID in addition: both snap bits; reach > GFT_EXCERPT_REACH_MAX; unknown flag bits. */
#define GFT_EXCERPT_WORDS 2u
#define GFT_EXCERPT_LINES 4u
#define GFT_EXCERPT_REACH_MAX 4096u
int gft_excerpt_spans_snap_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                  const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t before,
                                  uint32_t after, uint32_t flags, uint32_t reach, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off,
                                  uint64_t* d_exc_doc, uint32_t* d_exc_start, uint64_t* d_exc_span_off, uint64_t cap_exc, uint32_t* d_span_rel,
                                  uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes);
/* The host form of the snapped call, as gft_debug_excerpt_spans is of the plain one: the same header, the same walk. */
int gft_debug_excerpt_spans_snap(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                 const uint32_t* span_start, const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags,
                                 uint32_t reach, uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start,
                                 uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc,
                                 uint64_t* total_bytes);
/* The two edge walks on their own: the window [lo, hi) of the document doc[0, L), lo <= hi <= L, already clipped -> the snapped
 * window (the implied rune snap first, then the word or line snap).  GFT_E_INVALID as above, and for lo > hi or hi > L. */
int gft_debug_excerpt_snap_edges(const uint8_t* doc, uint64_t L, uint64_t lo, uint64_t hi, uint32_t flags, uint32_t reach, uint64_t* lo_out,
                                 uint64_t* hi_out);

/* ---- Highlight on the device: markers written round the hits (csrc/gft_mark.hip) --------------------------------------------
 * Between "where" (the spans) and "show it" (the excerpts): the text of a resident batch with `open` written in front of every
 * hit and `close` behind it -- <em> .. </em>, ** .. **, ANSI colour codes.  The text grows; the index outputs keep every call
 * behind this one usable on the marked text.  No scan, no dictionary, no programs; gft_last_nonascii is left alone.
 * Input: the batch under the scans' placement contract (no alignment, d_doc_off[0] may be non-zero, 64 readable bytes of slack;
 * neither the lead bytes nor the slack change the answer), and a span CSR as gft_hit_spans_device wrote it,
 * gft_map_spans_to_source_device rewrote it, or gft_excerpt_spans_device handed it back as (d_exc_span_off, d_span_rel,
 * d_span_len) for its blob.  open and close are HOST memory, 0 .. GFT_MARK_MAX bytes each, copied by the call; NULL is allowed
 * where the length is 0.  flags must be 0.
 * Runs: the runs of a document are the connected components of the union of its spans [start, start + len); spans that overlap,
 * nest, repeat or touch (a.end == b.start) are one run, a gap of one byte separates two; a run never crosses a document border.
 * By definition the runs are the excerpts gft_excerpt_spans_device forms for the same input with before = after = 0, flags = 0
 * (that call's d_exc_span_off, capped or not, names the runs' first spans by their indexes in the caller's span arrays);
 * a len == 0 span that touches nothing is a run of no bytes.  The order requirement is the excerpt's: within a document
 * start + len must not descend.  A batch that breaks it, or a span with start + len > L, is found on the device before anything
 * is written: GFT_E_INVALID, and nothing at all is written.
 * Output text: document d of L bytes with R(d) runs becomes its own bytes with open in front of the first byte of every run and
 * close behind its last: L + R(d) * (open_len + close_len) bytes.  A run of no bytes at p gets open and close back to back at p.
 * Nothing is inserted outside a document.  d_out holds the marked documents back to back in input order; with both lengths 0 it
 * is the batch's text byte for byte.
 * Index outputs, device memory, each nullable on its own, never capped, complete when given: d_out_off [n_docs + 1]
 * (d_out_off[0] = 0), the doc_off of d_out; d_span_new, parallel to d_span_start (the entries [d_span_off[0], d_span_off[n_docs])
 * are written): the span's start in its MARKED document, start + (r + 1) * open_len + r * close_len with r the index of the span's
 * run within its document; d_doc_run_off [n_docs + 1], the documents' CSR over the runs.  No marker lies inside a run, so
 * (d_out, d_out_off, n_docs, d_span_off, d_span_new, d_span_len) is a valid argument list of gft_redact_spans_device, of
 * gft_excerpt_spans_device and of this call itself: the order and the in-document checks hold on it.
 * Cap protocol of gft_compact_device: cap_bytes counts bytes of d_out; a byte at or past the cap is not written, be it text or
 * marker; nothing is stored at or past d_out + cap_bytes; d_out == NULL with cap_bytes == 0 counts only; GFT_OK either way, and
 * *n_runs / *total_bytes (host, nullable) are always handed back.
 * Launches on the engine's stream (gft_profile_read): "mark_runs" (the span checks, the suffix minimum and the heads: the
 * excerpt's passes), "mark_scan" (the prefix sum of the heads; the marked lengths checked), "mark_place" (d_out_off, d_span_new,
 * d_doc_run_off and the insertion list: 2 * n_runs blob positions, open at the even and close at the odd entries), "mark_copy"
 * (from the output side: a wave a 4 KiB tile, a lane a 16-byte chunk, the markers in LDS).  The call waits for the stream.
 * Between gft_process_device_begin and _end it is allowed only after _complete.  n_docs == 0 and no spans are valid: the output is
 * then a copy of the text.  GFT_E_UNSUPPORTED: a handle over several devices.  GFT_E_INVALID: flags != 0; a marker longer than
 * GFT_MARK_MAX; a non-zero length with a NULL marker; an output that overlaps an input or another output; document or span
 * offsets that descend; a document of 4 GiB or more, or one that would reach 4 GiB once marked (d_span_new is 32-bit).
 * GFT_E_NOMEM: no room for the work buffers (48 bytes a span, 16 a run).  Every refusal comes before any store, and the handle
 * stays usable after any error. */
#define GFT_MARK_MAX 255u   /* bytes of one marker */
int gft_mark_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                          const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len,
                          const uint8_t* open, uint32_t open_len, const uint8_t* close, uint32_t close_len, uint32_t flags,
                          uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint32_t* d_span_new, uint64_t* d_doc_run_off,
                          uint64_t* n_runs, uint64_t* total_bytes);
/* The host form, no HIP device needed, same contract, all pointers host (the 64 bytes of slack are not asked for here): the
 * runs by the excerpt's host walk, the copy tile by tile and lane by lane through the source the kernels are compiled from
 * (csrc/gft_mark_piece.hpp). */
int gft_debug_mark_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                         const uint32_t* span_start, const uint32_t* span_len, const uint8_t* open, uint32_t open_len,
                         const uint8_t* close, uint32_t close_len, uint32_t flags, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                         uint32_t* span_new, uint64_t* doc_run_off, uint64_t* n_runs, uint64_t* total_bytes);
/* where that walk's borders are: the spans of a tile of the suffix-minimum scan, the tiles of one carry trip, the bytes of a
 * lane's chunk of the output and of a wave's tile */
void gft_debug_mark_shape(uint32_t* tile_spans, uint32_t* trip_tiles, uint32_t* chunk_bytes, uint32_t* tile_bytes);

/* ---- Replace on the device: every hit run rewritten by its replacement (csrc/gft_replace.hip) --------------------------------
 * The fourth thing to do about a hit, beside masking it (gft_redact_spans_device), marking it (gft_mark_spans_device) and cutting
 * the text round it (gft_excerpt_spans_device): every run of hits becomes a placeholder -- [NAME], <host>, [KEY:aws] -- or is
 * deleted; strings.NewReplacer over the spans.  Every run changes the text by its own amount, which may be negative.  No scan, no
 * dictionary, no programs; gft_last_nonascii is left alone.
 * Input: the batch under the scans' placement contract (no alignment, d_doc_off[0] may be non-zero, 64 readable bytes of slack;
 * neither the lead bytes nor the slack change the answer), and a span CSR as gft_hit_spans_device wrote it,
 * gft_map_spans_to_source_device rewrote it, or the excerpt, the mark or this call handed it back for its own blob;
 * d_span_off[0] != 0 is valid.  The order rule and the in-document rule are the excerpt's: within a document start + len must not
 * descend, and start + len <= L.  flags must be 0.
 * Runs: gft_mark_spans_device's definition, word for word: the runs of a document are the connected components of the union of
 * its spans [start, start + len); spans that overlap, nest, repeat or touch (a.end == b.start) are one run, a gap of one byte
 * separates two; a run never crosses a document border; a len == 0 span that touches nothing is a run of no bytes.
 * The table, HOST memory, copied by the call: n_reps replacements, 1 .. 65536; replacement k is rep_bytes[rep_off[k] ..
 * rep_off[k + 1]), 0 .. GFT_REPLACE_MAX bytes, rep_off[0] == 0; length 0 deletes.  rep_bytes may be NULL when every length is 0.
 * Which replacement a span asks for: with d_span_key NULL (device, parallel to d_span_start: the entries [d_span_off[0],
 * d_span_off[n_docs]) are read) id 0; otherwise key = d_span_key[i], and the id is the key itself when key_rep is NULL and
 * key_rep[key] when it is given (HOST memory, n_keys entries, copied by the call; key < n_keys must hold).  The id must be below
 * n_reps.  d_span_term of gft_hit_spans_device is a valid d_span_key.  A run gets the SMALLEST id among its spans -- the table's
 * order is the priority --, which does not depend on the order of the spans in the list (the scan's canonical order is end
 * ascending: a run's first listed span is not its leftmost).
 * Output text: document d becomes its own bytes with every run replaced by its replacement; the bytes outside the runs are kept
 * byte for byte and in order; a run of no bytes at p gets its replacement inserted at p.  The documents stand back to back in
 * input order; a document's new length is L - (its runs' bytes) + (their replacements' bytes).
 * Index outputs, device memory, each nullable on its own: d_out_off [n_docs + 1] (d_out_off[0] = 0), the doc_off of d_out;
 * d_doc_run_off [n_docs + 1], the documents' CSR over the runs -- these two are never capped --; per run, in batch order and
 * capped by cap_runs: d_run_new, the replacement's first byte in its new document, d_run_len, the replacement's length, and
 * d_run_rep, the id chosen.  (d_out, d_out_off, n_docs, d_doc_run_off, d_run_new, d_run_len) is by construction a valid span
 * list of the redaction, the excerpt, the mark and this call on the replaced text: the placeholders can be highlighted, or the
 * text round them cut.
 * Cap protocol of gft_compact_device, two caps as in the excerpt call: cap_bytes counts bytes of d_out, cap_runs entries of the
 * three per-run arrays; nothing is stored at or past any array plus its cap; with all outputs NULL and both caps 0 the call only
 * counts; GFT_OK either way, and *n_runs / *total_bytes (host, nullable) are always handed back.
 * Launches on the engine's stream (gft_profile_read): "replace_runs" (the span checks, the suffix minimum and the heads: the
 * excerpt's passes), "replace_ids" (the prefix sum of the heads, every run's smallest id, the heads' replacement lengths),
 * "replace_scan" (the prefix sums of the runs' bytes and of the replacements' bytes; the new lengths checked), "replace_place"
 * (the index outputs and the plan: per run where its replacement begins in the output, the shift of the text behind it, its
 * length and its place in the table), "replace_copy" (from the output side: a wave a 4 KiB tile, a lane a 16-byte chunk; a table
 * of 4 KiB or less in LDS, a larger one read from L2).  The call waits for the stream.  Between gft_process_device_begin and _end
 * it is allowed only after _complete.  n_docs == 0 and no spans are valid: the output is then a copy of the text.
 * GFT_E_UNSUPPORTED: a handle over several devices.  GFT_E_INVALID: flags != 0; n_reps == 0 or above 65536; a replacement longer
 * than GFT_REPLACE_MAX; a rep_off that descends or has rep_off[0] != 0; a key >= n_keys or an id >= n_reps (found on the device,
 * like the order and the in-document violations); an output that overlaps an input or another output; document or span offsets
 * that descend; a document of 4 GiB or more, or one that would reach 4 GiB once replaced.  GFT_E_NOMEM: no room for the work
 * buffers (72 bytes a span, 24 a run, and the table: its bytes, 8 an entry, 4 a key).  Every refusal comes before any store, and
 * the handle stays usable after any error. */
#define GFT_REPLACE_MAX 255u   /* bytes of one replacement */
int gft_replace_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                             const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len,
                             const uint32_t* d_span_key, const uint32_t* key_rep, uint32_t n_keys, const uint8_t* rep_bytes,
                             const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes,
                             uint64_t* d_out_off, uint64_t* d_doc_run_off, uint32_t* d_run_new, uint32_t* d_run_len, uint32_t* d_run_rep,
                             uint64_t cap_runs, uint64_t* n_runs, uint64_t* total_bytes);
/* The host form, no HIP device needed, same contract, all pointers host (the 64 bytes of slack are not asked for here): the
 * runs by the excerpt's host walk, the copy tile by tile, trip by trip and lane by lane through the source the kernels are
 * compiled from (csrc/gft_replace_piece.hpp). */
int gft_debug_replace_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                            const uint32_t* span_start, const uint32_t* span_len, const uint32_t* span_key, const uint32_t* key_rep,
                            uint32_t n_keys, const uint8_t* rep_bytes, const uint64_t* rep_off, uint32_t n_reps, uint32_t flags,
                            uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_run_off, uint32_t* run_new,
                            uint32_t* run_len, uint32_t* run_rep, uint64_t cap_runs, uint64_t* n_runs, uint64_t* total_bytes);
/* where that walk's borders are: the spans of a tile of the suffix-minimum scan, the tiles of one carry trip, the bytes of a
 * lane's chunk of the output and of a wave's tile, the plan entries of a wave's window, the bytes of a table that goes into LDS */
void gft_debug_replace_shape(uint32_t* tile_spans, uint32_t* trip_tiles, uint32_t* chunk_bytes, uint32_t* tile_bytes, uint32_t* window,
                             uint32_t* lds_table);

/* ---- Term statistics on the device: how often each keyword hit, in how many documents, and where first -----------------
 * The histogram of a term list in CSR form on the engine's device: the entries of document d are d_term[d_off[d] .. d_off[d + 1]);
 * d_off[0] may be non-zero (a run of documents cut from a larger batch).  The arguments are (match_off, term_id) of
 * gft_scan_device -- with or without GFT_SCAN_UNIQUE --, or (d_span_off, d_span_term) of gft_hit_spans_device, of a selected or
 * routed blob too.  The call runs no scan, needs neither a dictionary nor programs and leaves gft_last_nonascii alone.
 * Output: three arrays of n_terms uint64, each nullable on its own (all three NULL only validates the input):
 *   d_occ[t]    the number of entries with term t
 *   d_docs[t]   the number of documents whose run holds t at least once
 *   d_first[t]  doc_base + the smallest such document, UINT64_MAX when there is none
 * Without GFT_STATS_ACCUMULATE the arrays are overwritten (untouched terms read 0, 0, UINT64_MAX).  With it the counts are added
 * to what the arrays hold and d_first becomes the minimum of what it holds and the new value: the statistics of a stream of
 * batches stay on the device, doc_base being the number of documents in front of this batch.  All counters are 64-bit end to end.
 * Launches on the engine's stream (gft_profile_read): "stats_check" (a descending offset, a term id >= n_terms: found on the
 * device before anything is written -- the list is not trusted, no atomic ever lands outside the counters), "stats_count" (a
 * workgroup a range of whole documents of near-equal weight; counts combined in LDS, one global atomic per workgroup, distinct
 * term and counter; csrc/gft_stats_piece.hpp).  The call waits for the stream.  Between gft_process_device_begin and _end it is
 * allowed only after _complete.  n_docs == 0, an empty list and n_terms == 0 (with an empty list) are valid.
 * GFT_E_UNSUPPORTED: a handle over several devices.  GFT_E_INVALID, before anything is written and with the three arrays byte for
 * byte as they were: an offset that descends; a term id >= n_terms; an output that overlaps an input or another output; a size
 * beyond the address space; unknown flag bits.  GFT_E_NOMEM: no room for the work buffers -- 16 bytes of flags, and, only with
 * n_terms above the bitset's LDS limit (gft_debug_stats_shape), ceil(n_terms / 32) * 4 bytes per workgroup of the count pass
 * (three per compute unit at most); nothing per entry.  The handle stays usable after any error. */
#define GFT_STATS_ACCUMULATE 1u
int gft_term_stats_device(gft_engine* e, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms,
                          uint32_t flags, uint64_t doc_base, uint64_t* d_occ, uint64_t* d_docs, uint64_t* d_first);
/* d_count[c] = the number of rows r with bit c set, for the n_cols columns of a bitmap in gft_process's layout (ceil(n_cols / 32)
 * words a row; finder rows and the group finder's rule rows alike).  Bits at and above n_cols are ignored, whatever they hold.
 * With d_row_idx (nullable) the counted rows are d_row_idx[0 .. n_rows), repeated indices counting repeatedly: the per-expression
 * counts of a routed bucket.  GFT_STATS_ACCUMULATE adds to d_count, without it the array is overwritten.  One launch
 * (gft_profile_read: "stats_columns"); overlap and size checks, GFT_E_UNSUPPORTED and the _complete rule as above. */
int gft_count_columns_device(gft_engine* e, const uint32_t* d_bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* d_row_idx,
                             uint32_t flags, uint64_t* d_count);
/* The statistics of a resident batch in one call: with d_hit_bitmap the KEPT matches -- gft_hit_spans_device in count-then-fill
 * form into buffers of the engine's, then the histogram of (span_off, span_term) --, with d_hit_bitmap == NULL every dictionary
 * match -- gft_scan_device's canonical CSR.  scan_flags: GFT_FOLD_ASCII or 0; n_terms is gft_n_terms.  It counts as a scan.
 * nonascii (nullable): set to 1, with NOTHING counted, when the scan folded and the batch was not fold-safe (gft_last_nonascii):
 * the caller lowers the batch and calls again -- an accumulating array never sees a batch twice.  With nonascii == NULL such a
 * batch is counted as scanned.
 * This call, gft_batch_top_docs_device and their whole-word twins refuse in one order, each under the name of the entry point that
 * was called, before anything is allocated or scanned: a null d_text_blob or d_doc_off with n_docs != 0 ("null argument"); unknown
 * bits in flags, then in scan_flags; for the top calls k above 4096, then k != 0 without both top arrays; a handle over several
 * devices (GFT_E_UNSUPPORTED); a handle without a device (GFT_E_HIP, "no HIP device available"); an n_docs beyond the address
 * space (2^60 or more; above 2^38 for the twins: "a size beyond the address space").  What the list's source and its consumer
 * refuse behind that -- a handle that is not built, batches in flight, the overlaps, the list's own faults -- they say in their
 * own words, as when called directly. */
int gft_batch_term_stats_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t flags, uint64_t doc_base, uint64_t* d_occ,
                                uint64_t* d_docs, uint64_t* d_first, int* nonascii);
/* The host forms, no HIP device needed, same contracts, all pointers host: the kernels' walks workgroup by workgroup, step by step
 * and lane by lane through the source they are compiled from (csrc/gft_stats_piece.hpp). */
int gft_debug_term_stats(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, uint32_t flags, uint64_t doc_base,
                         uint64_t* occ, uint64_t* docs, uint64_t* first);
int gft_debug_count_columns(const uint32_t* bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* row_idx, uint32_t flags,
                            uint64_t* count);
/* where those walks' borders are: the entries and the documents of a step at most, the slots of the step's set and of the
 * workgroup's cache (a term's slot is term mod cache_slots; the pairs (d, t) and (d, t + set_slots) meet in the set), the entries
 * at which a document takes the large path, the n_terms up to which its bitset lies in LDS, the weight (entries + documents) a
 * workgroup owns at least, the rows a workgroup of the column count owns */
void gft_debug_stats_shape(uint32_t* step_entries, uint32_t* step_docs, uint32_t* set_slots, uint32_t* cache_slots, uint32_t* large_entries,
                           uint32_t* bitset_lds_terms, uint32_t* range_weight, uint32_t* column_rows);

/* ---- Rank on the device: a score per document, the k best documents, documents by index list (csrc/gft_rank.hip) ----------
 * Which documents matched most.  All arithmetic is integer: every result is exact and reproducible.
 *
 * gft_score_docs_device.  The list is the CSR gft_term_stats_device takes -- (match_off, term_id) of gft_scan_device or (d_span_off,
 * d_span_term) of gft_hit_spans_device; d_off[0] may be non-zero.  d_score[d] = the sum of weights[t] over the entries of document
 * d; with GFT_SCORE_DISTINCT over the DISTINCT terms of d.  weights: HOST memory, n_terms words, copied by the call; NULL = every
 * term 1; a weight of 0 mutes a term.  Fewer than 2^32 entries of 32-bit weights cannot overflow the 64-bit sum.  Every one of the
 * n_docs scores is written, an empty document's is 0; *max_score (host, nullable) is the largest.  The call needs neither a
 * dictionary nor programs and leaves gft_last_nonascii alone.  Launches (gft_profile_read): "score_check" -- the statistics' check
 * pass: a descending offset or a term id >= n_terms is found on the device before anything is written --, "score_docs" -- the
 * statistics' walk (csrc/gft_stats_piece.hpp): a workgroup owns a range of whole documents of near-equal weight and walks it in
 * steps of whole documents whose sums lie in LDS; a document of large_entries entries or more is summed by a whole workgroup; the
 * distinct mode asks the step's set and the large path's bitset as the statistics' docs counter does.  A document has one owner:
 * its score goes out by a plain store, no atomic touches d_score, no workgroup waits for another.  The weights lie in LDS while
 * n_terms <= weight_lds_terms (gft_debug_rank_shape), above that they are read through the cache.  The call waits for the stream.
 * Refusals and rules are gft_term_stats_device's: GFT_E_INVALID with d_score byte for byte as it was (unknown flag bits, a
 * descending offset, a term id >= n_terms, d_score over an input, a size beyond the address space), GFT_E_UNSUPPORTED for a handle
 * over several devices, between _begin and _end only after _complete, the handle usable after any error.  Work buffers: 80 bytes
 * of control block, n_terms * 4 bytes of weights, in the distinct mode above bitset_lds_terms a bitset row per workgroup; nothing
 * per entry or document. */
#define GFT_SCORE_DISTINCT 1u
int gft_score_docs_device(gft_engine* e, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms,
                          const uint32_t* weights, uint32_t flags, uint64_t* d_score, uint64_t* max_score);
/* The k best of a score array.  The order is total: the larger score first, among equal scores the smaller document index first.  A
 * document whose score is 0 is never listed: *n_top (host) = min(k, number of non-zero scores).  d_top_idx[r] = doc_base + d and
 * d_top_score[r] its score for r < *n_top; the entries at and past *n_top are not written.  k <= 4096 (max_k: one workgroup's sort
 * in LDS, 16 bytes a candidate); a larger k is GFT_E_INVALID; k == 0 and n_docs == 0 are valid and list nothing.  d_score is any
 * uint64 array, not only one gft_score_docs_device wrote: nothing about it is trusted.  Launches: "top_max" (the largest score),
 * "top_select" -- a radix select over the 64-bit key, digit_bits bits a pass from the digit of the maximum's top bit down: a
 * histogram launch (LDS bins, one atomic per workgroup and non-empty bin) and a one-wave pick that leaves the prefix and the rank
 * still looked for in the control block, so the host reads nothing between the passes; with fewer than k documents there is no
 * k-th score and no select --, "top_place" (score above the threshold T, and the first k - c documents in index order with score
 * T, c the scores above it: ballots per tile of place_tile documents behind the tiles' prefix sums), "top_sort" (one workgroup, a
 * bitonic network in LDS).  No workgroup waits for another; the call waits for the stream.  Refusals as above, the two arrays byte
 * for byte as they were; an output over the scores or over the other output is one of them.  Work buffers: the control block, 16 KB
 * of histograms, 24 bytes per tile of place_tile documents (0.024 bytes a document) with the prefix sum's partials, 16 bytes a
 * candidate. */
int gft_top_docs_device(gft_engine* e, const uint64_t* d_score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* d_top_idx,
                        uint64_t* d_top_score, uint64_t* n_top);
/* Documents by index list: the output side of gft_select_docs_device for a list instead of a bitmap.  Output document j is input
 * document d_idx[j] - idx_base, in list order; repeats are allowed.  It materialises the top list, and any doc_idx a select, a route
 * or a context call returned, in any order.  d_out_off [m + 1] is complete whatever the cap; *total_bytes the bytes of the listed
 * documents.  Cap protocol, the 64 bytes of slack behind the text, the overlap refusals and the 4 GiB document limit are the
 * select's: nothing is stored at or past d_out + min(total, cap_bytes); d_out == NULL with cap_bytes == 0 counts only.  Launches:
 * "gather_place" (every index checked against n_docs on the device: an index outside -- or a listed document whose offsets descend
 * or that has 4 GiB or more -- is GFT_E_INVALID before a byte is written), "gather_scan", "gather_copy" (the select's copy pass).
 * Work buffers: 20 bytes per list entry. */
int gft_gather_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_idx,
                           uint64_t m, uint64_t idx_base, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* total_bytes);
/* Scores and top list of a resident batch in one call, as gft_batch_term_stats_device counts one: with d_hit_bitmap the KEPT matches
 * score (gft_hit_spans_device in count-then-fill form into buffers of the engine's), with NULL every dictionary match.  weights:
 * host, gft_n_terms words, or NULL.  d_score [n_docs] is nullable when only the list is wanted.  The select starts at the maximum
 * the score pass found.  nonascii as there: set to 1 with NOTHING written when the scan folded and the batch was not fold-safe.
 * The refusals in front of the scan and their order are written down there: k above 4096 and a missing top array are among them,
 * so no scan runs for a call that asks for them. */
int gft_batch_top_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                              const uint32_t* d_hit_bitmap, const uint32_t* want, const uint32_t* weights, uint32_t flags, uint32_t k,
                              uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx, uint64_t* d_top_score, uint64_t* n_top,
                              int* nonascii);
/* The host forms, no HIP device needed, same contracts, all pointers host: the kernels' walks step by step and lane by lane through
 * the source they are compiled from (csrc/gft_rank_piece.hpp). */
int gft_debug_score_docs(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights, uint32_t flags,
                         uint64_t* score, uint64_t* max_score);
int gft_debug_top_docs(const uint64_t* score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* top_idx, uint64_t* top_score,
                       uint64_t* n_top);
int gft_debug_gather_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* idx, uint64_t m, uint64_t idx_base,
                          uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* total_bytes);
/* where those walks' borders are: the entries and the documents of a step at most, the entries at which a document takes the large
 * path, the slots of the step's set, the n_terms up to which the weights and the large path's bitset lie in LDS, the weight a
 * workgroup owns at least, the bits of a select pass, the documents of a place tile, the largest k */
void gft_debug_rank_shape(uint32_t* step_entries, uint32_t* step_docs, uint32_t* large_entries, uint32_t* set_slots, uint32_t* weight_lds_terms,
                          uint32_t* bitset_lds_terms, uint32_t* range_weight, uint32_t* digit_bits, uint32_t* place_tile, uint32_t* max_k);

/* ---- Whole-word matching on the device: a match or span list filtered at word borders (csrc/gft_words.hip) -----------------
 * Every other call matches substrings: `he` fires inside `ushers`.  This one takes a list of occurrences in CSR form and the text
 * they were found in, keeps the entries that stand at word borders and compacts the list stably.
 * The rule.  A rune is a WORD rune when its Unicode general category starts with L, M or N, or is Pc -- letters, marks, numbers,
 * connector punctuation (`_`); the table is csrc/unicode_word.inc.  U+FFFD and every byte the decoder rejects are no word runes.
 * An occurrence is the bytes [s, e) of document D = text[doc_off[d] .. doc_off[d + 1]), s and e relative to the document; it is
 * KEPT iff
 *   NOT( word(utf8.DecodeLastRune(D[:s])) AND word(utf8.DecodeRune(D[s:e])) )   and
 *   NOT( word(utf8.DecodeLastRune(D[s:e])) AND word(utf8.DecodeRune(D[e:])) )
 * with Go's semantics: the strict decoder (overlong forms, surrogates, values above U+10FFFF are rejected), DecodeLastRune goes
 * back over at most UTFMax - 1 bytes to a rune start and gives RuneError unless the rune decoded there ends exactly at the slice's
 * end, an empty slice gives no rune and demands nothing.  So only a word rune against a word rune across an edge drops an
 * occurrence; a keyword edge that is no word rune demands nothing (`c++` is kept in `c++x`, `.net` in `asp.net`); an entry of
 * length 0 is kept; and nothing outside the document is ever looked at -- not the lead bytes, not the slack, not the neighbouring
 * document, not the other half of a rune that a document border cuts.
 * The list: the entries of document d are [d_off[d], d_off[d + 1]); d_off[0] may be non-zero (a run cut from a larger batch).
 * Entry i lies at d_pos[i] and is d_len[i] bytes long when d_len is given, d_term_len[d_term[i]] otherwise (d_term_len: n_terms
 * words on the device); d_term, when given, is carried through.  GFT_WORDS_POS_END: d_pos is the occurrence's LAST byte (the
 * positions of a GFT_POS_END engine), otherwise its first.  The arguments are (match_off, pos, NULL, term_id) of gft_scan_device
 * with the dictionary's lengths, or (span_off, span_start, span_len, span_term) of gft_hit_spans_device.
 * The text lies as gft_scan_device takes it: no alignment, d_doc_off[0] may be non-zero; every text byte is read on its own and
 * only inside its document.
 * Output: the kept entries of document d, in the order given, are [d_out_off[d], d_out_off[d + 1]) of d_out_pos (the position as
 * given), d_out_len (the length used) and d_out_term; d_out_off[0] = 0.  Cap protocol of gft_compact_device: cap counts entries;
 * an entry at or past cap is NOT written and nothing is stored at or past any array + cap; d_out_off (n_docs + 1 entries,
 * nullable, always complete when given) is not capped; all outputs NULL with cap == 0 counts only; GFT_OK in both cases and
 * *total (host, nullable) is always handed back.  d_out_len and d_out_term may each be NULL on their own; d_out_term needs d_term.
 * Launches on the engine's stream (gft_profile_read): "word_check" (the list is not trusted: an offset that descends, a term id
 * >= n_terms when the lengths come from the term table, an entry that leaves its document are found on the device before a text
 * byte is read or anything is written), "word_mark", "word_scan", "word_place".  The call waits for the stream.
 * GFT_E_INVALID, with every output byte as it was: the three findings of the check; an output that overlaps an input or another
 * output; unknown flag bits; a size beyond the address space.  GFT_E_UNSUPPORTED: a handle over several devices.  GFT_E_NOMEM: no
 * room for the work buffers (12 bytes an entry).  Between gft_process_device_begin and _end only after _complete.  Needs no
 * dictionary and no programs, leaves gft_last_nonascii alone; n_docs == 0 and an empty list are valid; the handle stays usable
 * after any error. */
#define GFT_WORDS_POS_END 1u
int gft_filter_word_matches_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_off,
                                   const uint32_t* d_pos, const uint32_t* d_len, const uint32_t* d_term, const uint32_t* d_term_len,
                                   uint32_t n_terms, uint32_t flags, uint64_t* d_out_off, uint32_t* d_out_pos, uint32_t* d_out_len,
                                   uint32_t* d_out_term, uint64_t cap, uint64_t* total);
/* gft_scan_device followed by the filter, into library-owned buffers (valid until the next call on the engine): the whole-word
 * matches of the batch as device pointers.  flags: GFT_FOLD_ASCII; GFT_SCAN_UNIQUE and GFT_POS_RUNES: GFT_E_INVALID.  It counts as a
 * scan (gft_last_nonascii).  With GFT_FOLD_ASCII the borders are judged on the text as it lies: folding A-Z changes no class. */
int gft_scan_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                          gft_matches* out_dev);
/* The bitmap of gft_process_device, computed from the whole-word matches alone: the scan with positions, the filter, then the
 * solver over the kept list as caller-supplied matches (slot = term id) while the scan's own units contribute nothing.
 * gft_process_again finds no scan to reuse afterwards; a gft_process_device on the same handle before or after answers as ever.
 * flags: GFT_FOLD_ASCII or 0.  GFT_E_UNSUPPORTED: a handle over several devices; a set of programs with an expression the host
 * solves (gft_n_host_exprs > 0 -- the host solver is not fed from the kept list).  There is no _begin / _end form.
 * gft_process_words is the host-buffer form (text_blob[0 .. doc_off[n_docs]) uploaded as gft_process uploads it). */
int gft_process_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                             uint32_t* d_hit_bitmap);
int gft_process_words(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, uint32_t* hit_bitmap);
/* gft_hit_spans_device with the whole-word rule: that call's spans, in count-then-fill form into buffers of the engine's, then the
 * filter into the caller's arrays -- same signature, same cap protocol, same refusals. */
int gft_hit_spans_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                               const uint32_t* d_hit_bitmap, const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off,
                               uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap, uint64_t* total);
/* gft_batch_term_stats_device over the whole-word matches: gft_hit_spans_words_device with a bitmap, gft_scan_words_device without */
int gft_batch_term_stats_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                      const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t flags, uint64_t doc_base, uint64_t* d_occ,
                                      uint64_t* d_docs, uint64_t* d_first, int* nonascii);
/* gft_batch_top_docs_device over the whole-word matches, the same way */
int gft_batch_top_docs_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                    const uint32_t* d_hit_bitmap, const uint32_t* want, const uint32_t* weights, uint32_t flags, uint32_t k,
                                    uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx, uint64_t* d_top_score, uint64_t* n_top,
                                    int* nonascii);
/* The filter on the host, no HIP device needed, same contract, all pointers host: the kernels' walk, entry tile by entry tile
 * through the source they are compiled from (csrc/gft_words_piece.hpp). */
int gft_debug_filter_word_matches(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* off, const uint32_t* pos,
                                  const uint32_t* len, const uint32_t* term, const uint32_t* term_len, uint32_t n_terms, uint32_t flags,
                                  uint64_t* out_off, uint32_t* out_pos, uint32_t* out_len, uint32_t* out_term, uint64_t cap, uint64_t* total);
/* 1 when cp is a word rune, 0 otherwise: 0 for surrogates, U+FFFD and every value above 0x10FFFF */
uint32_t gft_debug_word_rune(uint32_t cp);
/* where the walk's borders are: the entries a workgroup takes per step; the class table's rows of 256 bits and its bytes */
void gft_debug_words_shape(uint32_t* tile_entries, uint32_t* table_rows, uint32_t* table_bytes);

/* ---- finder.Finder mirror (finder/finder.go:32-240) ---------------------------------------------------------
 * Host-side orchestration with the reference's semantics: expression registry, keyword / regex sets, lazy engine
 * build with the same dirty flags (incl. the ForceBuild quirk, finder.go:218-235), error propagation, results in
 * registration order.  The DSL parser inside is dsl/parser.go + dsl/scanner.go restated (same trees, same error
 * strings).  All solving happens on the GPU (gft_process); text case folding follows strings.ToLower.
 * The substring engine defaults to the built-in GPU engine; foreign engines (any SubstringEngine / RegexEngine
 * implementation, e.g. Go's regexp behind RegexpEngine, or test mocks) are injected as callbacks. */
typedef struct gft_finder gft_finder;

/* emit one Match{Position, Term} (finder/finder.go:11-14) */
typedef void (*gft_emit_fn)(void* sink, const uint8_t* term, uint32_t term_len, int64_t position);
/* BuildEngine(keywords|regexes, caseSensitive): return 0, or non-zero with a NUL-terminated message in err */
typedef int (*gft_engine_build_fn)(void* user, const uint8_t* blob, const uint64_t* off, uint32_t n,
                                   int case_sensitive, char* err, uint32_t err_cap);
/* FindSubstrings / FindRegexes(text): call emit(sink, ...) per match; return 0, or non-zero with message */
typedef int (*gft_engine_find_fn)(void* user, const uint8_t* text, uint64_t text_len, gft_emit_fn emit, void* sink,
                                  char* err, uint32_t err_cap);

int gft_finder_create(gft_finder** out, int case_sensitive, int device); /* NewFinder(GpuEngine, EmptyRgxEngine, cs) */
/* the same finder over several devices (gft_engine_create_multi): finder.NewFinder(&GpuEngine{Devices: ...}, ...) */
int gft_finder_create_multi(gft_finder** out, int case_sensitive, const int* devices, int n_devices);
void gft_finder_destroy(gft_finder* f);
const char* gft_finder_last_error(const gft_finder* f);
gft_engine* gft_finder_engine(gft_finder* f); /* the GPU engine handle used for scanning/solving */
int gft_finder_set_substring_engine(gft_finder* f, gft_engine_build_fn build, gft_engine_find_fn find, void* user);
int gft_finder_set_regex_engine(gft_finder* f, gft_engine_build_fn build, gft_engine_find_fn find, void* user);
/* AddExpressionWithTag (finder.go:115-134).  GFT_E_PARSE + the reference's error text on malformed input. */
int gft_finder_add_expression(gft_finder* f, const uint8_t* expr, uint64_t expr_len, const uint8_t* tag,
                              uint64_t tag_len);
uint32_t gft_finder_n_expressions(const gft_finder* f);
/* which: 0 = keywords, 1 = regexes.  Returns the set size; item i via gft_finder_literal. */
uint32_t gft_finder_n_literals(const gft_finder* f, int which);
int gft_finder_literal(const gft_finder* f, int which, uint32_t i, const uint8_t** ptr, uint32_t* len);
/* expression i: its source string, tag and parsed tree as JSON ({"Type":..,"LExpr":..}); pointers valid until
 * the next call on f */
int gft_finder_expression(const gft_finder* f, uint32_t i, const uint8_t** str, uint32_t* str_len,
                          const uint8_t** tag, uint32_t* tag_len, const uint8_t** tree_json, uint32_t* json_len);
int gft_finder_force_build(gft_finder* f);                       /* ForceBuild (finder.go:218-235) */
/* ProcessText (finder.go:139-179): indices of the expressions that are true, in registration order. */
int gft_finder_process_text(gft_finder* f, const uint8_t* text, uint64_t text_len, uint32_t* out_idx, uint32_t cap,
                            uint32_t* n_true);
/* Batch extension: one bitmap row per document (layout as gft_process). */
int gft_finder_process_texts(gft_finder* f, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs,
                             uint32_t* hit_bitmap);
/* documents the host regex engine was called on by the last gft_finder_process_texts (the regex prefilter, SURVEY.md
 * 8(f) #3, sends it only documents that contain every required literal of some regex; GFT_REGEX_PREFILTER=0 disables) */
uint64_t gft_finder_last_regex_docs(const gft_finder* f);
/* Tags.  Distinct tags are numbered by first appearance in registration order; the empty tag of AddExpression
 * (finder.go:80-82) is a tag like any other.  The finder hands the tag id of every expression to its engine
 * (gft_set_expr_labels) whenever it sets the programs.  Pointers are valid until the next call on f. */
uint32_t gft_finder_n_tags(const gft_finder* f);
int gft_finder_tag(const gft_finder* f, uint32_t i, const uint8_t** ptr, uint32_t* len);
int64_t gft_finder_expression_tag_id(const gft_finder* f, uint32_t expr_i);   /* -1: no such expression */
/* The batch form of ProcessText's result: document d's true expressions are expr_idx[row_off[d] .. row_off[d + 1]) in
 * registration order, tag_id[k] the tag id of expression expr_idx[k].  Same semantics as gft_finder_process_texts (regex
 * prefilter, injected engines, the ToLower repeat of a batch that leaves ASCII, error propagation).  The three buffers are
 * library-owned and stay valid until the next call on f.  A batch whose bitmap is complete on the device is compacted there
 * and only these arrays are downloaded (gft_process_sparse). */
int gft_finder_process_texts_sparse(gft_finder* f, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs,
                                    const uint64_t** row_off, const uint32_t** expr_idx, const uint32_t** tag_id);
/* Same with the corpus resident in HBM (GPU substring engine, no regex terms).  A batch that leaves ASCII
 * (gft_last_nonascii) is lowered on the device into a buffer of the engine (gft_to_lower_device's kernels) and scanned again
 * from there: neither text nor bitmap crosses the link.  No device memory for that buffer: GFT_E_NOMEM.  GFT_DEVICE_TOLOWER=0
 * in the environment when the finder is created (and every finder over several devices): such a batch goes to the host
 * instead -- text down, ToLower per document, scan, bitmap up; the results are the same. */
int gft_finder_process_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                              uint32_t* d_hit_bitmap);
/* gft_split_lines_device on the finder's engine: the offsets of a resident blob of lines, for the call above.  It asks of the
 * finder what that call asks (the GPU substring engine, no regex terms) and refuses in its words. */
int gft_finder_split_lines_device(gft_finder* f, const uint8_t* d_blob, uint64_t len, uint32_t mode, uint64_t* d_doc_off, uint64_t cap,
                                  uint64_t* n_docs);
/* gft_select_docs_device on the finder's engine with n_cols = gft_finder_n_expressions: the documents of a resident batch whose
 * rows -- as the calls above leave them -- hit `want`.  It asks of the finder what gft_finder_process_device asks and refuses in
 * its words; no batch of gft_finder_process_device_begin may be in flight. */
int gft_finder_select_docs_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                  const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint8_t* d_out,
                                  uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs, uint64_t* n_selected,
                                  uint64_t* total_bytes);
/* gft_context_docs_device on the finder's engine with n_cols = gft_finder_n_expressions.  It asks of the finder what
 * gft_finder_select_docs_device asks and refuses in its words. */
int gft_finder_context_docs_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                   const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint64_t before,
                                   uint64_t after, const uint8_t* d_fence, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off,
                                   uint64_t* d_doc_idx, uint8_t* d_kind, uint64_t cap_docs, uint64_t* d_group_off, uint64_t cap_groups,
                                   uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups, uint64_t* total_bytes);
/* gft_route_docs_device on the finder's engine with n_cols = gft_finder_n_expressions.  It asks of the finder what
 * gft_finder_select_docs_device asks and refuses in its words. */
int gft_finder_route_docs_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                 const uint32_t* d_hit_bitmap, const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags,
                                 const uint8_t* d_also, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx,
                                 uint64_t cap_docs, uint64_t* bucket_doc, uint64_t* bucket_byte);
/* gft_hit_spans_device on the finder's engine under the finder's case rule, over the rows the calls above left.  A
 * case-insensitive finder passes GFT_FOLD_ASCII; when the batch is not fold-safe (gft_last_nonascii) it lowers the batch with the
 * gft_to_lower_device kernels and scans the lowered text, as gft_finder_process_device does, and sets *lowered = 1 (else 0).  A
 * LIMITATION: the spans then index the LOWERED text -- the bytes gft_to_lower_device gives for the batch, with its offsets --, not
 * the caller's text: lower-casing can change lengths, and no mapping back is built.  It asks of the finder what
 * gft_finder_process_device asks and refuses in its words; such a batch on a finder without the device ToLower
 * (GFT_DEVICE_TOLOWER=0): GFT_E_UNSUPPORTED.  gft_finder_hit_spans_source_device below has no such limitation. */
int gft_finder_hit_spans_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_hit_bitmap,
                                const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off, uint32_t* d_span_start, uint32_t* d_span_len,
                                uint32_t* d_span_term, uint64_t cap, uint64_t* total, int* lowered);
/* The same call, but the spans ALWAYS index the caller's text: when the batch was lowered, gft_map_spans_to_source_device runs over
 * the spans the call kept before it returns; *lowered still reports what happened.  Under the cap protocol only the entries that
 * were written (those below cap) are mapped and nothing is stored at or past cap.  The map reads the offsets and the lengths:
 * cap != 0 without d_span_off or without d_span_len is GFT_E_INVALID, whatever the batch holds (cap == 0 counts only, as above). */
int gft_finder_hit_spans_source_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                       const uint32_t* d_hit_bitmap, const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off,
                                       uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap, uint64_t* total,
                                       int* lowered);
/* gft_excerpt_spans_device on the finder's engine, behind one of the two calls above: spans_lowered is the *lowered that call
 * reported, source non-zero when it was the source form.  With source, or for a batch that was not lowered, the excerpts are cut
 * from the caller's batch (the mapped spans index it).  Otherwise the spans index the lowered text: the finder lowers the batch on
 * the device again, as it did for the scan, cuts the excerpts from that text and sets *lowered = 1 (else 0) -- d_exc_start and
 * d_span_rel are then positions of the lowered documents.  Everything else is gft_excerpt_spans_device's contract; the refusals of
 * gft_finder_process_device in its words. */
int gft_finder_excerpts_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                               const uint32_t* d_span_start, const uint32_t* d_span_len, int spans_lowered, int source, uint32_t before, uint32_t after,
                               uint32_t flags, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc, uint32_t* d_exc_start,
                               uint64_t* d_exc_span_off, uint64_t cap_exc, uint32_t* d_span_rel, uint64_t* d_doc_exc_off, uint64_t* n_exc,
                               uint64_t* total_bytes, int* lowered);
/* gft_excerpt_spans_snap_device on the finder's engine: gft_finder_excerpts_device with `reach`.  The rule for lowered batches
 * and `source` is unchanged: the snap judges the text the excerpts are cut from. */
int gft_finder_excerpts_snap_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                    const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, int spans_lowered,
                                    int source, uint32_t before, uint32_t after, uint32_t flags, uint32_t reach, uint8_t* d_out,
                                    uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc, uint32_t* d_exc_start, uint64_t* d_exc_span_off,
                                    uint64_t cap_exc, uint32_t* d_span_rel, uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes,
                                    int* lowered);
/* gft_mark_spans_device on the finder's engine, under the rule of gft_finder_excerpts_device: with source, or for a batch that
 * was not lowered, the caller's batch is marked; otherwise the finder lowers the batch on the device again, marks that text and
 * sets *lowered = 1 (else 0).  Everything else is gft_mark_spans_device's contract. */
int gft_finder_mark_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                           const uint32_t* d_span_start, const uint32_t* d_span_len, int spans_lowered, int source, const uint8_t* open,
                           uint32_t open_len, const uint8_t* close, uint32_t close_len, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes,
                           uint64_t* d_out_off, uint32_t* d_span_new, uint64_t* d_doc_run_off, uint64_t* n_runs, uint64_t* total_bytes,
                           int* lowered);
/* gft_replace_spans_device on the finder's engine, under the rule of gft_finder_mark_device: with source, or for a batch that was
 * not lowered, the caller's text is replaced; otherwise the finder lowers the batch on the device again, replaces in that text and
 * sets *lowered = 1 (else 0).  d_span_term: the term ids gft_finder_hit_spans_device wrote (device, nullable: id 0 for every
 * span); term_rep: HOST memory, gft_n_terms entries of the finder's engine, term -> replacement id, nullable -- NULL means id 0
 * for every term.  Everything else is gft_replace_spans_device's contract. */
int gft_finder_replace_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                              const uint32_t* d_span_start, const uint32_t* d_span_len, int spans_lowered, int source,
                              const uint32_t* d_span_term, const uint32_t* term_rep, const uint8_t* rep_bytes, const uint64_t* rep_off,
                              uint32_t n_reps, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_run_off,
                              uint32_t* d_run_new, uint32_t* d_run_len, uint32_t* d_run_rep, uint64_t cap_runs, uint64_t* n_runs,
                              uint64_t* total_bytes, int* lowered);
/* Term statistics of a resident batch on the finder's engine under the finder's case rule, as gft_finder_hit_spans_device runs:
 * a batch that leaves ASCII is lowered on the device first and *lowered set to 1 (term ids do not depend on positions: nothing is
 * mapped back).  d_hit_bitmap non-NULL: the statistics of the KEPT matches -- the witness occurrences of true, wanted expressions
 * (want: host words, NULL = every expression); NULL: of every dictionary match of the batch.  n_terms of the arrays is the
 * engine's (gft_n_terms of the finder's engine); flags, doc_base and the three arrays as gft_term_stats_device takes them.  The
 * refusals of gft_finder_hit_spans_device in its words. */
int gft_finder_term_stats_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                 const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t flags, uint64_t doc_base, uint64_t* d_occ,
                                 uint64_t* d_docs, uint64_t* d_first, int* lowered);
/* Scores and top list of a resident batch on the finder's engine (gft_batch_top_docs_device; with the whole-word option its words
 * twin) under the same case rule: a batch that leaves ASCII is lowered on the device first and *lowered set to 1 -- document indices
 * are the same in both forms, the list needs no mapping back.  weights: host, gft_n_terms of the finder's engine, or NULL; flags, k,
 * doc_base, d_score (nullable), the two top arrays and n_top as gft_batch_top_docs_device takes them.  The refusals of
 * gft_finder_term_stats_device. */
int gft_finder_top_docs_device(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                               const uint32_t* d_hit_bitmap, const uint32_t* want, const uint32_t* weights, uint32_t flags, uint32_t k,
                               uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx, uint64_t* d_top_score, uint64_t* n_top, int* lowered);
/* ... pipelined (gft_process_device_begin / _end): _end also lowers and repeats a batch that left ASCII, as above (a younger
 * batch in flight is completed in place first) */
int gft_finder_process_device_begin(gft_finder* f, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                    uint32_t* d_hit_bitmap);
int gft_finder_process_device_end(gft_finder* f);
/* Whole-word matching (gft_filter_word_matches_device above).  With the option on, on the same handle:
 * gft_finder_process_text / _texts / _texts_sparse go through gft_process_words (the sparse rows are compacted on the host),
 * gft_finder_process_device through gft_process_words_device, the repeat on the device-lowered text included,
 * gft_finder_hit_spans_device / _source_device through gft_hit_spans_words_device (the filter runs on the text that was scanned,
 * before the map back to the source), gft_finder_term_stats_device through gft_batch_term_stats_words_device.  The select, route,
 * redact, excerpt and mark calls take those calls' rows and spans and need nothing of their own.  With a foreign substring engine,
 * regex terms or an engine over several devices each of these calls gives GFT_E_UNSUPPORTED and says which of them is the cause;
 * gft_finder_process_device_begin gives GFT_E_UNSUPPORTED.  Off (the default) nothing changes. */
int gft_finder_set_whole_words(gft_finder* f, int on);
int gft_finder_whole_words(const gft_finder* f);
/* batches that gft_finder_process_device / _end have repeated because they left ASCII, by path */
int gft_finder_lowered_batches(const gft_finder* f, uint64_t* on_device, uint64_t* on_host);
/* gft_compact_device on the finder's engine (d_tag_id: the tag id of every entry, or NULL): pairs with
 * gft_finder_process_device, and with _begin / _end in the total == NULL form -- after a batch's _end has returned. */
int gft_finder_compact_device(gft_finder* f, const uint32_t* d_hit_bitmap, uint64_t n_docs, uint64_t* d_row_off,
                              uint32_t* d_expr_idx, uint32_t* d_tag_id, uint64_t cap, uint64_t* total);
/* test hooks mirroring what finder_test.go does by poking struct fields (finder/finder_test.go:205-217) */
int gft_finder_debug_add_literal(gft_finder* f, int which, const uint8_t* lit, uint32_t len);
int gft_finder_debug_set_updated(gft_finder* f, int updated_sub, int updated_rgx);
int gft_finder_debug_get_updated(const gft_finder* f, int* updated_sub, int* updated_rgx);

/* ---- Group finder: group/finder/finder.go + group/dsl on top of a finder --------------------
 * The tag-rule DSL and the object walk run on the host; every string leaf of every JSON document of a call becomes one
 * document of ONE batch through the finder (the reference runs one ProcessText per leaf, group/finder/internal.go:28-31).
 * Results are JSON documents written like the gft_dsl_* calls below (out/cap/needed). */
typedef struct gft_group gft_group;
int gft_group_create(gft_group** out, gft_finder* finder);      /* NewFinder(findthem) (finder.go:28-35); finder is borrowed */
void gft_group_destroy(gft_group* g);
const char* gft_group_last_error(const gft_group* g);
/* AddRule(ruleName, []string{expr}) (finder.go:45-66): GFT_E_PARSE + the reference's error text on malformed input */
int gft_group_add_rule(gft_group* g, const uint8_t* name, uint64_t name_len, const uint8_t* expr, uint64_t expr_len);
/* {"rules":{name:[{"ExpressionString":..,"Expression":{tree}}]},"fields":[..],"tags":[..]} (the struct finder_test.go compares) */
int gft_group_state(const gft_group* g, char* out, uint64_t cap, uint64_t* needed);
/* ProcessJson (what = 0, finder.go:160-172) / TagJson (what = 1, finder.go:80-92) over a batch of raw JSON documents
 * (blob + offsets).  include/exclude: JSON arrays of path prefixes, or NULL.  Output: one element per document,
 * {"rules":{rule:[expressions]}} / {"tags":{tag:{field:[expressions]}}} or {"error":"..."} */
int gft_group_process_jsons(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs,
                            const uint8_t* include_json, uint64_t include_len, const uint8_t* exclude_json,
                            uint64_t exclude_len, int what, char* out, uint64_t cap, uint64_t* needed);
/* the document of the last gft_group_process_jsons call again (it is kept, so a too-small buffer costs no second run) */
int gft_group_last_result(const gft_group* g, char* out, uint64_t cap, uint64_t* needed);
/* EvaluateRules (finder.go:118-137) on a caller-supplied {tag:{field:[expressions]}} map -> {rule:[expressions]} */
int gft_group_evaluate(gft_group* g, const uint8_t* tagmap_json, uint64_t len, char* out, uint64_t cap, uint64_t* needed);
/* string leaves and text bytes the last gft_group_process_jsons call sent through the finder (measurement) */
int gft_group_last_batch(const gft_group* g, uint64_t* leaves, uint64_t* bytes);
/* ---- Records: a batch that is columns of strings already, rules evaluated on the device (gft_rules.hip) ------------
 * A schema is F unique field paths, byte strings as the object walk builds them ("Body", "Meta.Notes", "items.index(2)",
 * "" for the TagText case); include / exclude as in gft_group_process_jsons, exclude wins.  A batch is N records in CSR
 * form over leaves: record r owns the leaves rec_off[r] .. rec_off[r + 1], leaf l lies in field leaf_field[l] of the
 * schema and holds the bytes leaf_off[l] .. leaf_off[l + 1] of text_blob (64 readable bytes behind the text, as for every
 * scan).  A record may have no leaves and may name a field more than once; an empty string is a leaf.  The result is
 * rule_bitmap[r * ceil(R / 32) + (i >> 5)] bit (i & 31) = rule expression i is true for record r -- what EvaluateRules of
 * TagObject gives for an object with exactly those (path, string) leaves.  Rule expressions are numbered by ascending rule
 * name (byte order), AddRule order inside a name.
 * The rules are compiled against the schema here (a refusal leaves the previous schema and its set answering) and again,
 * lazily, once rules or finder expressions have been added.  GFT_E_UNSUPPORTED names the limit: more than 65535 fields,
 * more than 8192 distinct (tag, field path) units, an expression that needs an operand stack deeper than 32. */
int gft_group_set_schema(gft_group* g, const uint8_t* paths_blob, const uint64_t* path_off, uint32_t n_fields,
                         const uint8_t* include_json, uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len);
uint32_t gft_group_n_rule_exprs(gft_group* g);
/* rule name and expression string of bit i; the pointers stay valid until the next gft_group_add_rule */
int gft_group_rule_expr(gft_group* g, uint32_t i, const uint8_t** name, uint32_t* name_len, const uint8_t** expr, uint32_t* expr_len);
/* Every pointer is a device pointer.  The leaves go through gft_finder_process_device (its limits apply: GPU substring
 * engine, no regex terms, one device; a batch that leaves ASCII is lowered and scanned again on the device) into a bitmap
 * the engine owns, then the two rule kernels run on the engine's stream; only the status crosses the link.  GFT_E_INVALID:
 * no schema, a leaf_field entry >= F, rec_off that descends or does not end at n_leaves, leaves but no records (also for a
 * group without rules: both calls check the same things).  GFT_E_NOMEM: no room for the work buffers.  n_records == 0,
 * n_leaves == 0 and a group without rules are valid.  Groups that share a finder may be called from several threads: a
 * call holds the engine from the install of its rule set to the end. */
int gft_group_process_records_device(gft_group* g, const uint8_t* d_text_blob, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field,
                                     const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap);
/* Host pointers.  A finder that qualifies for the call above: upload, that call, the rule bitmap back.  Any other finder
 * (regex terms, injected engines): the leaf bitmap comes from gft_finder_process_texts and is uploaded to the same kernels.
 * Both routes give the same rows; a finder error is the call's error. */
int gft_group_process_records(gft_group* g, const uint8_t* text_blob, const uint64_t* leaf_off, const uint32_t* leaf_field,
                              const uint64_t* rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap);
/* The compiled device words (field masks, units, postfix programs) interpreted on the host over a caller-supplied leaf
 * bitmap [n_leaves][ceil(n_exprs / 32)]; n_exprs must be the finder's number of expressions.  Needs no device. */
int gft_debug_eval_rules(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                         uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap);
/* The same two kernels that gft_group_process_records_device runs, over a caller-supplied leaf bitmap on the device (every
 * pointer is a device pointer): what the kernels make of rows the finder did not write.  Bits at and above n_exprs in a
 * row's last word are ignored.  One device; validation as for the call above. */
int gft_debug_eval_rules_device(gft_group* g, const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field,
                                const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap);
/* ---- Tag entries: TagObject / TagJson on the device as sparse (field, expression) lists (gft_tags.hip) ----------------------
 * For a record batch under the schema, the tag map of every record -- tag -> field path -> {expression}, finder.go:87-110 -- comes
 * back as three columns:
 *     row_off   u64 [n_records + 1]   record r owns the entries row_off[r] .. row_off[r + 1]
 *     ent_field u32 [total]           schema index of the leaf's field
 *     ent_expr  u32 [total]           finder expression index
 *     ent_tag   u32 [total]           nullable: the tag id of expression ent_expr (gft_finder_expression_tag_id)
 * Inside a record the leaves come in record order (rec_off[r] .. rec_off[r + 1]), inside a leaf the expression index ascends.
 * A leaf contributes one entry per set bit e < n_exprs of its hit row (bits at and above n_exprs in a row's last word are
 * ignored), and only when its field is valid: isValidateFieldPath under the schema's include / exclude lists, exclude wins.
 * (The host route drops invalid leaves before the finder sees them; the device decoder keeps them, the mask is applied here.)
 * A record that names a field twice contributes twice: nothing is de-duplicated or sorted on the device.  The tag map is a map
 * of sets, so the consumer's insert removes the duplicate, and records decoded from JSON never repeat a field (GFT_JSON_DUP).
 * {(tag of ent_expr, schema[ent_field], ExpresionStr of ent_expr)} over a record's entries is TagObject's map for an object with
 * exactly those (path, string) leaves.  A group without rules is valid; a finder without expressions gives total = 0.
 * Cap protocol, as for gft_compact_device and gft_group_json_leaves_device: row_off is always complete; an entry at a position
 * >= cap is not stored and nothing is stored past the caps; the status is GFT_OK either way; *total (host memory, nullable)
 * receives row_off[n_records]; NULL arrays with cap == 0 count only.
 * Validation, as for gft_group_process_records_device: GFT_E_INVALID for no schema, a leaf_field entry >= F, rec_off that
 * descends or does not end at n_leaves, leaves but no records -- such leaves and records are skipped on the device, never
 * dereferenced, and the handle goes on answering.  Handles over several devices: GFT_E_UNSUPPORTED from the device-pointer
 * calls.  GFT_E_NOMEM: no room for the work buffers (counts, offsets and scan partials of their own, grown on demand).
 *
 * Every pointer is a device pointer except total.  The leaves go through gft_finder_process_device into the engine's leaf
 * bitmap (the limits of gft_group_process_records_device), then three launches run on the engine's stream (gft_profile_read:
 * "tags_count", "tags_scan", "tags_fill"); only the status and the total cross the link. */
int gft_group_tag_records_device(gft_group* g, const uint8_t* d_text_blob, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field,
                                 const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field,
                                 uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap, uint64_t* total);
/* Host pointers.  A finder that qualifies for the call above: upload, that call into arrays the engine owns, the arrays down.
 * Any other finder (regex terms, injected engines, several devices): the leaf bitmap comes from gft_finder_process_texts and
 * the entries are made on the host.  Both routes give the same arrays; a finder error is the call's error. */
int gft_group_tag_records(gft_group* g, const uint8_t* text_blob, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                          uint64_t cap, uint64_t* total);
/* Device pointers: gft_group_json_leaves_device into buffers the engine owns, then gft_group_tag_records_device over them, a
 * document a record.  d_status [n_docs] as in gft_group_process_jsons_device: a document whose status is not 0 has an empty row. */
int gft_group_tag_jsons_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                               uint64_t* d_row_off, uint32_t* d_ent_field, uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap,
                               uint64_t* total);
/* Host pointers; the same result document as gft_group_process_jsons(..., what = 1) with the include / exclude lists given to
 * gft_group_set_schema: upload, the documents decoded and tagged on the device, the status down; the documents of status != 0
 * (and those of more than GFT_TAGS_JSON_MAX_LEAVES string values) go through gft_group_process_jsons' route as one sub-batch and
 * take its "tags" or "error"; the document itself is written on the device from the leaf rows where they are
 * (gft_group_tags_json_device, the host-decided documents as holes) and comes down as one piece of text: the entries never cross
 * the link.  GFT_DEVICE_RESULT=0, read when the group is created, tables the format cannot hold, or no device memory for the
 * text: the entries of gft_group_tag_jsons_device come down instead and every document of status 0 gets {"tags": ..} from them on
 * host threads -- the same bytes.  A finder that does not qualify (regex terms, injected engines, several devices) takes
 * gft_group_process_jsons' route for the whole batch.  gft_group_last_result and gft_group_json_last serve this call too. */
int gft_group_tag_jsons_schema(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, char* out, uint64_t cap,
                               uint64_t* needed);
/* TagJson as the reference has it: no schema.  As gft_group_process_jsons_auto -- the schema discovered from the batch, kept
 * between calls (one kept schema serves both calls) -- with the result document of gft_group_process_jsons(..., what = 1).  A
 * limit that refuses the discovered schema is never the caller's error: the batch takes the host route. */
int gft_group_tag_jsons_auto(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* include_json,
                             uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap,
                             uint64_t* needed);
/* The contract above stated in plain loops on the host over a caller-supplied leaf bitmap [n_leaves][ceil(n_exprs / 32)]; n_exprs
 * must be the finder's number of expressions.  Needs no device.  It is also the second route of gft_group_tag_records. */
int gft_debug_tag_entries(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                          uint64_t cap, uint64_t* total);
/* The three launches of gft_group_tag_records_device over a caller-supplied leaf bitmap on the device (every pointer is a device
 * pointer except total): what the kernels make of rows the finder did not write. */
int gft_debug_tag_entries_device(gft_group* g, const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field,
                                 const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field,
                                 uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap, uint64_t* total);
/* ---- JSON decoded on the device (gft_json.hip): raw documents in HBM -> the record form above ----------------------------
 * The schema of gft_group_set_schema is compiled into a trie of path components (split at '.', the root is the path "");
 * a wave walks a document in 64-byte pieces and resolves every object key and array element ("index(<i>)") in that trie,
 * exactly: a hash hit is confirmed by comparing the bytes; a key that contains '.' resolves to nothing.  The walker is exact
 * for every document it decides, and says which ones it did not decide -- one status byte per document: */
enum gft_json_status {
    GFT_JSON_OK = 0,     /* decided on the device: its leaves are those of the host route, byte for byte, in document order */
    GFT_JSON_SYNTAX = 1, /* the walker did not accept the text (the host route has the error text) */
    GFT_JSON_DEPTH = 2,  /* more than 32 containers open at once */
    GFT_JSON_PATH = 3,   /* a string value at a path that is not a schema path */
    GFT_JSON_KEY = 4,    /* an object key that is empty, contains a backslash or is not valid UTF-8 */
    GFT_JSON_DUP = 5,    /* a node of the trie was reached twice: a duplicate key at or above a schema path */
    GFT_JSON_TEXT = 6    /* a string value at a schema path with a \uD800..\uDFFF escape or a byte that is not valid UTF-8 */
};
/* A document with a status other than 0 contributes no leaves: its record is empty.  When several conditions hold the lowest
 * status is reported.  Status 0 is guaranteed for a document that is valid JSON (every number form, literal, escape; no
 * control byte in a string; nothing behind the top-level value), has at most 32 containers open at any point, whose keys are
 * non-empty valid UTF-8 without backslashes and do not repeat inside one object, whose string values all lie at schema paths
 * and consist of valid UTF-8, the escapes \" \\ \/ \b \f \n \r \t and \uXXXX outside D800..DFFF (\u0000 becomes a NUL byte
 * of the leaf).  Numbers, literals, and containers under keys the schema does not know carry no leaf: they are checked and
 * skipped.  A document that is not valid JSON never gets status 0.
 * Limits, answered by the calls of this section only (gft_group_set_schema accepts such schemas): GFT_E_UNSUPPORTED for a
 * schema with more than 16384 trie nodes (distinct path prefixes), or a path component longer than 65535 bytes.
 *
 * Every pointer is a device pointer except totals.  Three launches on the engine's stream (gft_profile_read: "json_count",
 * "json_scan", "json_write"); the contract mirrors gft_to_lower_device: d_status [n_docs] and d_rec_off [n_docs + 1] are always
 * complete; leaf l is written to d_leaf_field [leaf_cap] and d_leaf_off [leaf_cap + 1] when l < leaf_cap, a text byte when its
 * position is < text_cap, and nothing is stored past the caps (d_leaf_off[n_leaves] = the text's size is written when
 * n_leaves <= leaf_cap); GFT_OK is returned in both cases and totals[2] (host, nullable) receives the number of leaves and of
 * text bytes -- the caller compares and calls again.  NULL arrays with zero caps count only.  The decoded text is never
 * longer than the raw documents; the caller leaves 64 readable bytes behind it before handing it to a scan.  d_json_blob must
 * be readable for 64 bytes past d_doc_off[n_docs].  GFT_E_INVALID: no schema, offsets that descend, a document of 4 GiB or
 * more, output that overlaps the input.  Handles over several devices: GFT_E_UNSUPPORTED.  n_docs == 0 is valid. */
int gft_group_json_leaves_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                                 uint64_t* d_rec_off, uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text,
                                 uint64_t text_cap, uint64_t* totals);
/* The call above into buffers the engine owns (grown until the batch fits), then gft_group_process_records_device over them
 * (its limits apply): only the status and the totals cross the link.  d_rule_bitmap [n_docs][ceil(R / 32)]: the row of a
 * document whose status is not 0 is that of an empty record -- the caller consults d_status [n_docs]. */
int gft_group_process_jsons_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                                   uint32_t* d_rule_bitmap);
/* Host pointers; the same result document as gft_group_process_jsons(..., what = 0) with the include / exclude lists given to
 * gft_group_set_schema: upload, the call above, the status down; the documents of status != 0 go through
 * gft_group_process_jsons' route as one sub-batch and take its "rules" or "error"; the document itself is written on the device
 * from the rows where they are (gft_group_rules_json_device, the host-decided documents as holes) and comes down as one piece of
 * text.  GFT_DEVICE_RESULT=0, read when the group is created, or rules whose fragment table the format cannot hold: the rows
 * come down instead and every document of status 0 gets {"rules": ..} from its row on host threads -- the same bytes.  A finder
 * that does not qualify for the device record route (regex terms, injected engines, several devices) takes
 * gft_group_process_jsons' route for the whole batch.  gft_group_last_result serves this call too. */
int gft_group_process_jsons_schema(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, char* out, uint64_t cap,
                                   uint64_t* needed);
/* documents of the last gft_group_process_jsons_schema / _auto batch decided on the device / handed to the host route */
int gft_group_json_last(const gft_group* g, uint64_t* n_device, uint64_t* n_host);
/* ---- The result document of rule rows, written on the device (gft_result.hip) ------------------------------------------------
 * d_rule_bitmap [n_docs][ceil(R / 32)], as gft_group_process_jsons_device and gft_group_process_records_device leave it, ->
 * the text '[' D0 ',' D1 ... ']' with Dd = {"rules":{"<rule>":["<expression>",..],..}}: a member per rule with a set bit, rules
 * and expressions in bit order (gft_group_rule_expr), names and expressions escaped as gft_group_process_jsons escapes them; a
 * row without bits gives {"rules":{}}; bits at and above R in a row's last word are ignored.  It is byte for byte the result
 * document of gft_group_process_jsons(..., what = 0) for documents with those rule hits.  A caller with a resident blob gets
 * the document without the rows crossing the link.  A group without rules is valid: every document is {"rules":{}}.
 * d_out_off [n_docs + 1]: d_out_off[0] = 1, d_out_off[d + 1] = d_out_off[d] + len(d) + 1; the separator behind document d (','
 * or the closing ']') is the byte at d_out_off[d + 1] - 1.  n_docs == 0: "[]", *total = 2.
 * d_hole_len [n_docs], nullable: a value != 0 reserves exactly that many bytes for document d -- none of them is written and
 * its row is not read (the caller fills in a text of its own, an {"error": ..} for instance; every real document has at least
 * 12 bytes).  GFT_E_INVALID for a hole of 4 GiB or more.
 * Cap protocol of gft_compact_device: d_out_off is always complete, a byte at a position >= cap is not stored and nothing is
 * stored at or past d_out + cap, GFT_OK either way, *total (host memory, nullable) receives the text's size; d_out == NULL with
 * cap == 0 counts only.  Every pointer but total is a device pointer.  Three launches on the engine's stream (gft_profile_read:
 * "result_count", "result_scan", "result_fill"); the table of escaped names and expressions depends on the rules only -- no
 * schema is needed -- and is uploaded again when rules were added.  Handles over several devices: GFT_E_UNSUPPORTED, also for
 * rules whose escaped text does not fit 32-bit offsets.  GFT_E_NOMEM: no room for the work buffers. */
int gft_group_rules_json_device(gft_group* g, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out,
                                uint64_t cap, uint64_t* d_out_off, uint64_t* total);
/* The contract above stated in plain loops on the host (host pointers) over the group's current rules.  Needs no device and no
 * schema. */
int gft_debug_rules_json(gft_group* g, const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap,
                         uint64_t* out_off, uint64_t* total);
/* ---- The tag result document, written on the device (gft_tagdoc.hip) ----------------------------------------------------------
 * A leaf bitmap d_hit_bitmap [n_leaves][ceil(E / 32)] (E = the finder's expressions, as gft_finder_process_device leaves it over
 * the leaves as documents) with the record arrays of gft_group_tag_records_device -> the text '[' D0 ',' D1 ... ']' with
 * Dd = {"tags":{"<tag>":{"<field path>":["<expression>",..],..},..}}: a member per tag matched in a valid field of record d, tags
 * ascending bytewise; inside it a member per such field, paths ascending bytewise; inside that the distinct expression strings of
 * the tag that are true in the field, ascending bytewise; everything escaped as gft_group_process_jsons escapes it.  A record
 * without such a hit gives {"tags":{}}; bits at and above E are ignored; a leaf whose field the include / exclude lists take out
 * contributes nothing.  It is byte for byte the result document of gft_group_process_jsons(..., what = 1) for documents with
 * those leaves.  The order is compiled into tables once -- a slot per distinct (tag, expression string), a rank per field -- so no
 * entry is sorted: four launches on the engine's stream (gft_profile_read: "tagdoc_slots", "tagdoc_count", "tagdoc_scan",
 * "tagdoc_fill").  Needs a schema (gft_group_set_schema); the tables are uploaded again when expressions were added or the schema
 * changed.
 * d_out_off, d_hole_len, the cap protocol, n_records == 0 and total: exactly those of gft_group_rules_json_device (every real
 * document has at least 11 bytes).
 * GFT_E_INVALID: what gft_group_tag_records_device refuses of a batch, a hole of 4 GiB or more.  GFT_E_UNSUPPORTED -- "serialise
 * on the host", the handle answers afterwards --: a record that names a valid field twice, a record of more than
 * GFT_TAGS_JSON_MAX_LEAVES leaves that is not a hole, a document whose length + 1 does not fit 32 bits, tables whose escaped
 * text does not fit 32-bit offsets, handles over several devices.  GFT_E_NOMEM: no room for the work buffers (n_leaves times the
 * slot row's words among them). */
#define GFT_TAGS_JSON_MAX_LEAVES 1024
int gft_group_tags_json_device(gft_group* g, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                               uint64_t n_records, uint64_t n_leaves, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                               uint64_t* d_out_off, uint64_t* total);
/* The contract above stated in plain loops on the host (host pointers); n_exprs must be the finder's number of expressions.
 * Needs no device. */
int gft_debug_tags_json(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                        uint64_t n_records, uint64_t n_leaves, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off,
                        uint64_t* total);
/* ---- The schema discovered from the batch (gft_json.hip: k_json_paths) ------------------------------------------------------
 * One more pass of the same walker, without a trie, collects the distinct paths of the batch's string values on the device:
 * a set of 2^16 64-bit path hashes (linear probing), at most 16384 paths, a pool of 8 MiB for their bytes.  A path is spelled
 * as the object walk spells it ("Body", "Meta.Notes", "items.index(2)", "" for a top-level string); none is produced below a
 * key that is empty, contains a backslash or is not valid UTF-8, below 32 open containers, or when it is longer than 65535
 * bytes.  A value under a key that contains '.' is reported, its key as one component.  A path that the pass misses -- a hash
 * collision, a full set, the cap, the pool: *dropped counts the paths found and not kept -- only makes the documents that use
 * it GFT_JSON_PATH under the resulting schema: a miss costs time, never a result.  A document that is not valid JSON may
 * have contributed the paths in front of its error.
 *
 * Device pointers in (no byte outside the documents is read), host memory out: paths_blob [blob_cap] and
 * path_off [path_cap + 1] receive the paths sorted bytewise, each once; needed[2] (nullable): bytes, paths; GFT_E_INVALID when a
 * cap is too small (8 MiB and 16384 always suffice).  One launch on the engine's stream (gft_profile_read: "json_paths").  Needs
 * no schema.  GFT_E_INVALID: offsets that descend, a document of 4 GiB or more, a null argument.  Handles over several
 * devices: GFT_E_UNSUPPORTED.  n_docs == 0 is valid and gives no paths. */
int gft_group_json_paths_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* paths_blob,
                                uint64_t blob_cap, uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths, uint64_t* dropped);
/* ProcessJson as the reference has it: no schema.  Host pointers; the same result document as gft_group_process_jsons(...,
 * what = 0) with the same lists, for every batch.  The batch is uploaded once, its paths are discovered (the call above),
 * compiled into a schema of the group's own -- kept between calls and apart from gft_group_set_schema's, which goes on
 * answering its calls -- and gft_group_process_jsons_schema's route runs on the staged batch.  A later call compiles again only
 * when it found a path the kept schema lacks, when the lists changed, or when rules or finder expressions were added.  The
 * whole batch takes gft_group_process_jsons' route when the finder does not qualify (regex terms, injected engines, several
 * devices) or when the discovered schema is beyond a limit (16384 trie nodes, 65535 fields, ...): never an error of the
 * caller.  gft_group_last_result and gft_group_json_last serve this call too. */
int gft_group_process_jsons_auto(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* include_json,
                                 uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap,
                                 uint64_t* needed);
/* JSON Lines from host memory: one blob, a document a line (gft_split_lines_device, GFT_SPLIT_JSON_LINES).  With a schema set
 * (gft_group_set_schema) the result document of gft_group_process_jsons_schema -- the include / exclude arguments must then be
 * empty: GFT_E_INVALID --, without one that of gft_group_process_jsons_auto with these lists; both over the documents of the
 * split, byte for byte.  The blob is uploaded once and cut where it lies; the offsets come down at 8 bytes a document (the host
 * route needs them for the documents whose status is not 0) and the schema / auto route continues from the resident blob.  A
 * finder that does not qualify for the device route (regex terms, injected engines, several devices) splits on the host -- the
 * code behind gft_debug_split_lines -- and takes gft_group_process_jsons' route.  A blob without a non-blank line gives "[]".
 * gft_group_last_result and gft_group_json_last serve this call too. */
int gft_group_process_json_lines(gft_group* g, const uint8_t* blob, uint64_t len, const uint8_t* include_json, uint64_t include_len,
                                 const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap, uint64_t* needed);
/* what the last gft_group_process_jsons_auto found: distinct paths, paths found and not kept, 1 when it compiled a schema */
int gft_group_json_auto_last(const gft_group* g, uint64_t* n_paths, uint64_t* dropped, uint64_t* recompiled);
/* No device needed (tests), host pointers, the output contract of gft_group_json_paths_device: the discovery mode of the
 * kernels' walker on the host, 64-byte piece by piece, with the set and the pool as plain arrays (hashes [hash_cap], nullable:
 * the values in the set, ascending; *n_hashes: how many there are) -- ... */
int gft_debug_emulate_json_paths(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* paths_blob,
                                 uint64_t blob_cap, uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths, uint64_t* dropped,
                                 uint64_t* hashes, uint64_t hash_cap, uint64_t* n_hashes);
/* ... and the reference: the host route's JSON reader plus a walk that collects every string value's path as a list of
 * components, joined at the end, by code that shares nothing with the walker.  Only documents that the reader accepts count. */
int gft_debug_json_paths_ref(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* paths_blob, uint64_t blob_cap,
                             uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths);
/* No device needed (tests), host pointers, the array contract of gft_group_json_leaves_device: the reference -- the host
 * route's JSON reader and a walk of the decoded value against the schema, classified into the statuses above by code that
 * shares nothing with the walker -- ... */
int gft_debug_json_leaves_ref(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status, uint64_t* rec_off,
                              uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap, uint64_t* totals);
/* ... and the kernels' walker on the host, 64-byte piece by piece through the source the kernels are compiled from
 * (csrc/gft_json_walk.hpp): count, prefix sums, write */
int gft_debug_emulate_json_leaves(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status,
                                  uint64_t* rec_off, uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap,
                                  uint64_t* totals);
/* the trie's lookup: the child of node `parent` (0: the root) under one path component, or `parent` itself for key_len == 0;
 * -1: none.  *field (nullable): the node's field index, or -1 */
int64_t gft_debug_json_schema_find(gft_group* g, int64_t parent, const uint8_t* key, uint32_t key_len, int64_t* field);
/* group DSL alone (host only): {"tree":..,"tags":[..],"fields":[..]} or {"error":..}; token list as gft_dsl_tokens */
int gft_group_dsl_parse(const uint8_t* expr, uint64_t len, char* out, uint64_t cap, uint64_t* needed);
int gft_group_dsl_tokens(const uint8_t* expr, uint64_t len, char* out, uint64_t cap, uint64_t* needed);

/* ---- DSL front-end alone (host only, no device needed) ------------------------------------------------------
 * Each writes a NUL-terminated JSON document into out (cap bytes) and the size it needs into *needed; returns
 * GFT_OK, or GFT_E_INVALID when cap is too small (call again with *needed bytes).
 *   gft_dsl_parse : {"tree":{...},"keywords":[..],"regexes":[..],"program":[..]} or {"error":"<reference text>"};
 *                   "program" uses slots = index into keywords ++ regexes (first-seen order).
 *   gft_dsl_tokens: [{"Tok":"AND","Lit":"and","Err":null}, ...] up to and including EOF or the first error
 *                   (dsl/scanner.go:79-106).
 *   gft_to_lower  : strings.ToLower of the input (raw bytes out, not JSON). */
int gft_dsl_parse(const uint8_t* expr, uint64_t len, int case_sensitive, char* out, uint64_t cap, uint64_t* needed);
int gft_dsl_tokens(const uint8_t* expr, uint64_t len, char* out, uint64_t cap, uint64_t* needed);
/* the literal runs every match of an RE2-syntax pattern must contain, as a JSON array (empty: the pattern cannot be
 * prefiltered) -- what the finder's regex prefilter adds to the device dictionary */
int gft_regex_required_literals(const uint8_t* pattern, uint64_t len, char* out, uint64_t cap, uint64_t* needed);
int gft_to_lower(const uint8_t* in, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* needed);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------------- */
/* on = 1: every kernel launch is bracketed by HIP events on the engine's stream (categories "scan", "solve", "aux");
 * on = 2: the scan kernel's launches only -- an event record is a node of its own on the stream, a few microseconds
 * between two kernels: a run that is being timed as a whole brackets the one kernel it prices; 0: off. */
int gft_profile_enable(gft_engine* e, int on);
/* Sums since the last reset.  names: "scan", "solve", "aux".  Synchronises the stream. */
int gft_profile_read(gft_engine* e, const char* name, double* total_ms, uint64_t* launches);
int gft_profile_reset(gft_engine* e);

/* ---- several devices behind one handle ------------------------------------------------------ */
/* A handle over n_devices HIP devices (devices == NULL / n_devices == 0: every visible device).  It is used exactly like
 * a single-device handle -- gft_build, gft_set_programs, gft_scan, gft_process, gft_process_again and the gft_finder_*
 * functions on top of it --: tables and programs are replicated, a batch is cut into contiguous document ranges of
 * near-equal text bytes, every device has its own host thread and stream for the duration of a call, results land in the
 * caller's buffers in document order.  The *_device entry points of such a handle run on its first device; shards that
 * are already resident on their devices go through gft_process_device_multi.  A device may be named twice (tests). */
int gft_engine_create_multi(gft_engine** out, const int* devices, int n_devices);
int gft_n_devices(const gft_engine* e);
/* how gft_process_device_multi moves the shards' bitmaps to the first device: "rccl" (ncclSend / ncclRecv over xGMI),
 * "copy" (device-to-device copies: RCCL unavailable, or a device named twice) or "" (single-device handle).
 * GFT_RCCL_SELF=1 in the environment when the handle is created: a list that names ONE device several times gets one
 * communicator of one rank and the gather is that rank's grouped ncclSend / ncclRecv to itself ("rccl") -- how the RCCL
 * branch is exercised on a one-GPU box (tests/test_gpu_multi.py). */
const char* gft_gather_mode(const gft_engine* e);
gft_engine* gft_device_engine(gft_engine* e, int i);     /* the per-device engine (its stream, its profile counters) */
/* the document cuts gft_process would use: device i gets documents [cut[i], cut[i+1]); cut has n_devices + 1 entries */
int gft_split_docs(const gft_engine* e, const uint64_t* doc_off, uint64_t n_docs, uint64_t* cut);
/* Device-resident shards: d_text[i] / d_doc_off[i] / n_docs[i] live on device i (64 bytes of readable slack behind every
 * blob).  Every device scans and solves its shard; then the path's ONE exchange step gathers the bitmaps into
 * d_bitmap_root on the first device, shard after shard (sum(n_docs) x ceil(n_exprs / 32) words): ncclSend / ncclRecv in
 * one group over xGMI on communicators from ncclCommInitAll (device-to-device copies if RCCL is not available). */
int gft_process_device_multi(gft_engine* e, const uint8_t* const* d_text, const uint64_t* const* d_doc_off, const uint64_t* n_docs,
                             uint32_t flags, uint32_t* d_bitmap_root);

/* ---- test hook: the table compiler without a device ------------------------------------------------------- */
/* Compiles `terms` into the scan kernel's tables on the host and walks them over ONE document the way the kernel does
 * (host emulation of the per-probe logic, csrc/scan3_tables.cpp): the matches of the unit [lo, len) of the document, in no
 * particular order, as (term id in sorted-unique order, position) pairs.  No HIP device is needed; tests use it to check
 * the table compiler against the oracle.  *needed = number of matches (GFT_E_INVALID when cap is too small). */
int gft_debug_emulate_scan(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* text,
                           uint32_t len, uint32_t lo, uint32_t flags, uint32_t scan_flags, uint32_t* out_term,
                           uint32_t* out_pos, uint64_t cap, uint64_t* needed);

/* The two-positions-per-probe filter of gft_scan5.hip alone, on the host: compiles `terms` (suffix-window tables, then the
 * 3-gram filter over `groups` merged byte classes; 0 = as many as the dictionary has) and walks ONE document the way the
 * kernel's lanes do -- a probe at every even offset from `lane_start` answers that position from the low word and the next
 * one from the high word.  out_exact[i] / out_dual[i] = 1 when the one-probe-per-byte filter of gft_scan2.hip / this filter
 * flags a window ending at byte i.  The second must flag whatever the first flags (and is equal to it when no classes are
 * merged); *groups_used = the number of groups.  The first is computed from the bucket table's keys and the short terms
 * themselves, so any alphabet is served.  GFT_E_UNSUPPORTED when the dictionary has no suffix-window tables at all.
 * No HIP device is needed. */
int gft_debug_scan5_filter(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* text, uint32_t len,
                           uint32_t lane_start, uint32_t scan_flags, uint32_t groups, uint8_t* out_exact, uint8_t* out_dual,
                           uint32_t* groups_used);

/* The table set alone, on the host (csrc/table_set.cpp): compiles `terms` with the function gft_build calls -- or, when
 * `blob` is not NULL, reads that blob with the function gft_import_tables calls (the terms are ignored) --, chooses the scan
 * kernel the way both do for a device with `lds_max` bytes of LDS per workgroup (160 KiB on gfx950) and writes the set with
 * the function gft_export_tables calls.  forced_kernel: what GFT_SCAN_KERNEL would say (NULL: the environment's own value);
 * the GFT_SCAN5_* switches are read from the environment as usual.  *kernel = the chosen kernel's name (a static string),
 * *needed = the size of the written blob, copied into out when out is not NULL (GFT_E_INVALID when cap is too small);
 * err (nullable, err_cap bytes) receives the text of a refusal, whose status is returned.  No HIP device is needed and no
 * handle is built; tests use it to check the blob format, its validation and the table of DESIGN.md 4.7. */
int gft_debug_tables(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* blob, uint64_t blob_len,
                     uint64_t lds_max, const char* forced_kernel, const char** kernel, uint8_t* out, uint64_t cap, uint64_t* needed,
                     char* err, uint64_t err_cap);
/* What the handle has learnt from the batches it completed (read-only): *unit_max = the bytes per work unit that the next
 * call of a kernel on scan2's tables (scan2, scan5) runs with (8 192 after gft_build, down to 512 behind dense batches;
 * the other kernels do not read it), *fifo_cap (nullable) = the fifo entries that `learn` sizes it by. */
int gft_debug_learned_unit(const gft_engine* e, uint32_t* unit_max, uint32_t* fifo_cap);
/* How the last batch that the handle launched got its table of work units (read-only; *name is a static string): "host"
 * (computed on the host and uploaded: up to 1 024 documents from host memory), "counted" (counted on the device and the count
 * read back: a handle's first batches, gft_scan_device, a batch that is run again), "deferred" (filled into the table as the
 * batch before left it, the count read afterwards) or "single" (one launch on the assumption of one unit per document, after
 * two such batches); "" before the first batch.  A batch that was deferred and then run again reports the second run. */
int gft_debug_last_unit_route(const gft_engine* e, const char** name);
/* Who answered gft_last_nonascii for the batch whose entry point returned last (read-only): *bits = the word the scan kernels
 * left in the control block.  0: no byte >= 0x80 in a folded scan (or no folded scan); 2: the scan kernel judged the pieces with
 * high bytes itself and found the text unsafe (gft_scan3, gft_scan5); bit 0 set: high bytes were seen and not judged -- the DFA
 * kernel always, the other two when a unit listed more pieces than its candidate list holds -- and the second pass over the
 * text (k_fold_safe, k_fold_doc_edges) gave the verdict.  The tests use it to tell which of the judges they are testing. */
int gft_debug_last_fold_bits(const gft_engine* e, uint32_t* bits);
/* ... and the numbers of the plan that plan_scan makes for `terms`, compiled the same way: *kernel as above,
 * plan[0..3] = the longest keyword's bytes, then the shape of scan5's fifo entries (s5_term_bits, s5_pos_bias: term id and
 * relative position in 32 bits; both 0 under another kernel) and the entries of a wave's LDS match fifo, which the unit size
 * follows (gft_debug_learn's fifo_cap).  No HIP device is needed and no handle is built. */
int gft_debug_scan_plan(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint64_t lds_max, const char* forced_kernel,
                        const char** kernel, uint32_t* plan);
/* The entries that the scan of the handle's last completed batch wrote to the match pool (the scan kernel's own count, as the
 * batch's verdict read it back; a batch of gft_process_device_begin counts once its _end has returned).  With positions
 * (gft_scan*, or any INORD group among the expressions) that is the number of matches.  Without them the pool is read as a
 * set of terms per work unit, and k_scan5 writes the terms of a short-term record (the terms of one to three bytes that end
 * at one 3-window; the direct table of alphabets of up to 32 byte classes) once per unit, however often the window occurs
 * at end offsets >= 3 of the document; occurrences that end at offsets 0..2 and terms of four bytes or more are written
 * every time. */
int gft_debug_pool_entries(const gft_engine* e, uint64_t* entries);
/* The solver launch of the last batch (read-only): *pf_terms = the prefetch depth its plan chose (6 or 12; 0 before the first
 * solver launch), *unit_entries (nullable) = what the handle has learnt for the NEXT plan: the mean pool entries per work unit
 * of the last completed batch, rounded up (0: none yet, or nothing matched). */
int gft_debug_last_solve_pf(const gft_engine* e, uint32_t* pf_terms, uint32_t* unit_entries);

/* The judgement on a batch alone, on the host (csrc/batch_verdict.cpp): decodes the seven 64-bit words of a control-block
 * read-back and judges them against what a deferred scan launch knew -- single / epoch (its unit table came from the
 * one-launch path, which raises the block's flags to that number), n_docs, and the unit_cap, pool_cap and static_slabs IT
 * ran with -- by the very functions gft_process_device and _end call.  *kind = 0 accept, 1 run again the general way, 2 run
 * again with a match pool of *pool_need entries (0 otherwise), 3 invalid (its text in err, nullable, err_cap bytes);
 * verdict[6] = nonascii, nonascii bits, text_lo, text_hi, n_units, total.  No HIP device is needed and no handle. */
int gft_debug_judge_batch(const uint64_t* ctl_words, int single, uint32_t epoch, uint64_t n_docs, uint64_t unit_cap, uint64_t pool_cap,
                          uint64_t static_slabs, int* kind, uint64_t* pool_need, uint64_t* verdict, char* err, uint64_t err_cap);
/* ... and what a completed batch of `total` matches over the text range [text_lo, text_hi) teaches the next ones under
 * `kernel` ("dfa" .. "scan5"; fifo_cap: entries of a wave's LDS match fifo, ordered: the GFT_SCAN_ORDERED path): *unit_max
 * (bytes per work unit on scan2's tables) and *scan4_density go in as they were and come out as learnt. */
int gft_debug_learn(const char* kernel, uint32_t fifo_cap, int ordered, uint64_t total, uint64_t text_lo, uint64_t text_hi,
                    uint32_t* unit_max, double* scan4_density);

/* The solver's program compiler alone, on the host: the set is compiled by the very function gft_set_programs calls
 * (csrc/program_set.cpp: check, fusion with Sethi-Ullman operand order, control-bit device words, evaluation order, blocks of
 * 64 transposed) and every expression is then interpreted, from the transposed array the kernel reads, for ONE document
 * whose presence set is `present` (one byte per slot, non-zero = the slot's term occurs).  out_hit[i] = the expression's
 * truth value, out_depth[i] (nullable) = the accumulator-stack depth its fused form needs.  An expression that the device
 * does not answer from presence alone is GFT_E_UNSUPPORTED: an INORD group of more than one leaf (it needs positions), a
 * wide INORD group, an expression the host solves.  A program whose PUBLIC postfix form is deeper than 128 but whose fused
 * form is not is evaluated, as gft_set_programs accepts it.  GFT_E_INTERNAL: a program reaches a stack depth that the
 * interpreter chosen for its block does not have.  No HIP device is needed; tests use it to check the compiler against the
 * oracle's tree evaluation. */
int gft_debug_eval_programs(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots,
                            const uint8_t* present, uint8_t* out_hit, uint32_t* out_depth);
/* ... and what the solver's plan reads of the set so compiled, without evaluating it (so also for sets with INORD groups):
 * out_shape (shape_cap words; 3 + max(1, ceil(n_exprs / 64)) are written, GFT_E_INVALID if that is more) = words of the fused
 * programs, 1 if some program holds a NOT or INORD word, pairs of the widest wide INORD group, then the interpreter class
 * (0 flat, 1 two registers, 2 deep) of every block of 64 sorted programs (one entry for an empty set). */
int gft_debug_program_shape(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots, uint32_t* out_shape,
                            uint32_t shape_cap);

/* The solver's launch plan alone, on the host (csrc/solve_plan.cpp): plan_solve -- the function every gft_process* calls -- for
 * a program set of that shape (n_slots rows of the presence matrix, n_exprs, fprog_words, has_rare, wide_pairs: see
 * gft_debug_program_shape) on a device of n_cus CUs and lds_max bytes of LDS per workgroup, for a batch of n_docs documents, under
 * what GFT_SOLVE_GROUP_DOCS (forced_group, -1: unset), GFT_SOLVE_PROG_LDS (prog_lds) and GFT_SOLVE_DEBUG (dbg) would say.
 * plan[11] = group_docs, p_in_lds, prog_in_lds, rare (0 / 1 / 2), dbg_variant, tile_words, wide_cap, lds_bytes, per_cu, grid,
 * and 1 if the library carries the kernel of that plan (the launch table's own lookup).  No HIP device, no handle. */
int gft_debug_plan_solve(uint32_t n_slots, uint32_t n_exprs, uint32_t fprog_words, int has_rare, uint32_t wide_pairs,
                         uint64_t lds_max, uint32_t n_cus, uint64_t n_docs, int forced_group, int prog_lds, uint32_t dbg,
                         uint64_t* plan);

/* The same with what decides the prefetch depth of the presence-matrix build: unit_entries, the mean pool entries per unit of the
 * last completed batch (0: unknown), and forced_pf, what GFT_SOLVE_PF_TERMS would say (0: unset, 6 or 12; anything else is
 * GFT_E_INVALID).  plan[12] = the eleven words of gft_debug_plan_solve, then pf_terms (6 or 12). */
int gft_debug_plan_solve_pf(uint32_t n_slots, uint32_t n_exprs, uint32_t fprog_words, int has_rare, uint32_t wide_pairs,
                            uint32_t unit_entries, uint64_t lds_max, uint32_t n_cus, uint64_t n_docs, int forced_group, int prog_lds,
                            uint32_t dbg, uint32_t forced_pf, uint64_t* plan);

/* The host solver alone (csrc/host_solve.cpp: dsl/expression.go:66-142 restated over the postfix words, lists materialised):
 * Solve of ONE program over ONE document's map, given as n_lists keys -- slots[k] with the positions
 * positions[list_off[k] .. list_off[k+1]) in the order addMatchesToSolverMap appended them (a key may have no position at
 * all: it is present all the same, dsl/expression_test.go:29-33).  *out = 1 / 0.  This is what gft_process* runs for the
 * (expression, document) pairs the device does not answer itself: expressions beyond the device solver's limits, and INORD
 * expressions over a slot whose list is not ascending (a keyword and a regex with the same literal).  No device needed. */
int gft_debug_host_solve(const uint32_t* words, uint64_t len, const uint32_t* slots, const uint64_t* list_off,
                         const int64_t* positions, uint32_t n_lists, int* out);

#ifdef __cplusplus
}
#endif
#endif /* GFT_H */
