/*
 * sctools_hip.h — C ABI of libsctools_hip.so, the MI355X (gfx950) barcode hot path.
 *
 * The reference (dpeerlab/sctools) is pure Python and has no FFI of its own; each
 * entry point below replaces the Python function cited next to it, and the Python
 * drop-in (sctools_amd.encodings / sctools_amd.barcode) binds them with ctypes
 * (INTEGRATION.md shows the binding).  Conventions:
 *   - every function returns an int status: SCT_OK (0) or a negative SCT_E_* code;
 *     sct_last_error() returns a thread-local message for the last failure;
 *   - "device" functions take device pointers and a hipStream_t passed as void*
 *     (NULL = the default stream) and are asynchronous on that stream;
 *   - "_host" functions take host pointers, run on the current device and return
 *     only when results are back in host memory;
 *   - codes wider than 64 bits are `words` little-endian uint64 limbs per record
 *     (limb 0 holds bits 0..63 of the Python int);
 *   - no function retains a caller pointer after it returns (plans own their
 *     device buffers and hold no host pointers).
 */
#ifndef SCTOOLS_HIP_H
#define SCTOOLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_OK 0
#define SCT_E_INVALID (-1)   /* bad argument (maps to ValueError)             */
#define SCT_E_HIP (-2)       /* HIP runtime failure / no device (RuntimeError) */
#define SCT_E_NOMEM (-3)     /* device allocation failed (MemoryError)         */
#define SCT_E_RANGE (-4)     /* value outside what the kernel supports         */
#define SCT_E_INTERNAL (-5)  /* a bound the library's own code guarantees was passed (RuntimeError) */

/* ---------------------------------------------------------------- library */
int sct_version(void);                 /* ABI version, currently 1 */
const char* sct_last_error(void);      /* thread-local, never NULL */
int sct_device_count(int* count);      /* HIP devices visible to this process */
int sct_set_device(int device);        /* select the device for later calls (hipSetDevice) */

/* Launch-shape knobs.  None changes a result: they cut work into other chunk / grid sizes
 * or pick between index layouts that give identical outputs, so tests can put seams inside
 * small problems and benchmarks can sweep.  Process-global; the library reads no environment
 * variable.  value < 0 restores the default.  Read when a plan is created (scalar: per call). */
#define SCT_TUNE_SPECTRAL_CHUNK 1       /* slices per seed/tile pass (default 262144, the whole space; 65536 for SCT_ALLPAIRS_NO_CACHE plans) */
#define SCT_TUNE_SPECTRAL_MIN_N 2       /* AUTO takes SPECTRAL from this many 16-base codes (325000) */
#define SCT_TUNE_ALLPAIRS_GRAB 3        /* pair kernel: work items per queue pull */
#define SCT_TUNE_ALLPAIRS_FLUSH_ITEMS 4 /* pair kernel: flush lane counters every k items */
#define SCT_TUNE_ALLPAIRS_GRID 5        /* pair kernel: persistent grid size */
#define SCT_TUNE_NEAREST_SCHEME 6       /* 0 auto, 1 open addressing, 2 CSR buckets, 3 half keys */
#define SCT_TUNE_NEAREST_LOAD 7         /* CSR buckets per distinct block value (default 4); the open-addressing load is fixed at <= 1/2 */
#define SCT_TUNE_SCALAR_SERVER 8        /* 0: every scalar call is a kernel launch (default 1) */
#define SCT_TUNE_SCALAR_IDLE_MS 9       /* the scalar server exits after this idle time (5) */
#define SCT_TUNE_SPECTRAL_COLUMNS 10   /* SPECTRAL column width: 0 auto, 14, or 16 (when int8 fits) */
#define SCT_TUNE_PLAN_CACHE 11          /* 0: every all-pairs plan allocates its own buffers (default 1) */
#define SCT_TUNE_ENCODE_GRID 12         /* tiled encoder grid: 1 one workgroup per tile (default), 0 resident workgroups */
#define SCT_TUNE_INGEST_TILES 13        /* whitelist / FASTQ extraction: tiles per workgroup (0: one range per
                                           resident slot, the whitelist's default; FASTQ default 8) */
#define SCT_TUNE_FASTQ_ONEPASS 14       /* retired in round 5 (the one-pass FASTQ forms lost their A/B and were
                                           removed); accepted and ignored, so the key numbers stay stable */
#define SCT_TUNE_INGEST_DIRECT 15       /* whitelist ingest: up to this many 16 KiB tiles (4096) the encode pass
                                           sums the per-tile counts itself, no reduction launch */
#define SCT_TUNE_INGEST_SPEC 16         /* whitelist ingest: 1 tries 16-base lines in one read first (default), 0 never */
#define SCT_TUNE_COUNT_PREAGG 17        /* counter insert: 0 one table row per code, 1 equal codes of a wave merged
                                           first (default), 2 a per-workgroup LDS table per tile; the molecule
                                           counter's insert has the same three forms and default */
#define SCT_TUNE_COLLAPSE_FORM 18       /* UMI collapse: 0 one lane per table slot probes the molecule's 3 * L
                                           neighbours, 1 a wave shares one molecule's neighbours (default) */
#define SCT_TUNE_MERGE_ROWS 19          /* molecule merge on one device: 0 the kernel reads the source's table in
                                           place (default), 1 the source's rows are compacted and copied first, as
                                           they always are between two devices */
#define SCT_TUNE_TILE_CHAIN 20          /* SPECTRAL int8 tile, densest column <= 125 codes: 1 stage 2 as one MFMA
                                           chain per tile (default), 0 the shift form (read at plan creation) */
#define SCT_TUNE_DIRECTIONAL_FORM 21    /* directional clusters: 1 the sweeps run over the worklist of molecules
                                           with an in-edge (default), 0 every sweep runs over the whole table */
#define SCT_TUNE_DOWNSAMPLE_WAVE_READS 22 /* downsampling: a molecule of at least this many reads is thinned by its
                                           whole wave, 64 draws at a time (default 64); below it by its own lane */
#define SCT_TUNE_NKEYS 23
int sct_tune_set(int key, int64_t value);
int sct_tune_get(int key, int64_t* value);  /* -1 when unset */

/* ---------------------------------------------------------------- encoders
 * kind = 2 (TwoBit) or 3 (ThreeBit).
 * Replaces TwoBit.encode  (src/sctools/encodings.py:75-88, map :53-69) and
 *          ThreeBit.encode (src/sctools/encodings.py:155-167, map :139-149).
 * n records of L bytes, record r starting at seqs + r*stride (stride >= L).
 * codes : n*words uint64, words = ceil(kind*L/64) (at least 1); MSB-first packing
 *         exactly as the reference's `encoded <<= bits; encoded += map[byte]`.
 * gc    : nullable; n uint8 = GC count of the record (requires L <= 255).
 *         TwoBit: C/c/G/g bytes (the ambiguous positions are counted after the
 *         host fills them, see flags). ThreeBit: popcount of bit 0 of each triplet
 *         (encodings.py:182-192), i.e. C/c/G/g bytes.
 * flags : nullable (TwoBit); n uint8, bit0 = an IUPAC-ambiguous byte was seen
 *         (encoded as 0, to be drawn by the caller's random.randint(0,3) in order,
 *         encodings.py:69), bit1 = an invalid byte was seen (reference raises
 *         KeyError, encodings.py:68).  ThreeBit never flags (any byte -> N=6).
 */
int sct_encode(int kind, const uint8_t* seqs, int64_t n, int64_t stride, int L,
               uint64_t* codes, uint8_t* gc, uint8_t* flags, void* stream);
int sct_encode_host(int kind, const uint8_t* seqs, int64_t n, int64_t stride, int L,
                    uint64_t* codes, uint8_t* gc, uint8_t* flags);

/* Host-resident stream of n records (stride L, one limb: L <= 32 TwoBit / 21 ThreeBit):
 * chunks of `chunk` records (<= 0: 16M) pipeline H2D / encode / D2H over 3 streams.  Buffers
 * already page-locked (sct_host_pinned) are copied by DMA in place; pageable ones go through
 * the library's own pinned stage in chunks of <= 2M records (the library never registers
 * caller memory).  gc and flags are required.  Returns when all outputs are in host memory.
 * Replaces the per-record loop of encodings.py:60-71 / 140-147 for a batch of records. */
int sct_encode_stream_host(int kind, const uint8_t* seqs, int64_t n, int L, uint64_t* codes,
                           uint8_t* gc, uint8_t* flags, int64_t chunk);

/* *pinned = 1 when all of [p, p + bytes) lies in one page-locked host allocation the HIP
 * runtime knows (hipHostMalloc, torch pin_memory, hipHostRegister): the host-stream entry
 * points then DMA to / from it in place; 0 otherwise (pageable memory, or a range that
 * runs past its allocation). */
int sct_host_pinned(const void* p, int64_t bytes, int* pinned);

/* Page-locked host blocks (hipHostMalloc) for the Python layer's pinned array pool: the host
 * stream paths (FASTQ pieces read from files, their extracted rows, stream-encoded codes,
 * nearest results) then cross PCIe by DMA in place, and a block handed back to the pool is
 * reused without new page faults.  sct_host_free(NULL) is a no-op. */
int sct_host_alloc(int64_t bytes, void** ptr);
int sct_host_free(void* ptr);

/* Variable-length records (device): record r = starts[r] .. starts[r] + lens[r] of buf,
 * encoded as encodings.py:75-88 / :155-167 do into `words` limbs (words >= ceil(kind*len/64)
 * for every record); gc (nullable, saturating at 255) and flags as sct_encode. */
int sct_encode_var(int kind, const uint8_t* buf, const int64_t* starts, const int32_t* lens, int64_t n,
                   int words, uint64_t* codes, uint8_t* gc, uint8_t* flags, void* stream);

/* ---------------------------------------------------------------- whitelist ingest
 * Replaces the line loop of Barcodes.from_whitelist (src/sctools/barcode.py:95-97): the
 * file opened 'rb', every line (ending at '\n'; a final line may lack it) chopped by
 * `line[:-1]` (its last byte, whatever it is) and TwoBit-encoded.
 * sct_lines (device, synchronous): starts / lens (the chopped length) of every line; a
 * call with max_lines < the line count only reports *nlines (and *max_len = 0).
 * sct_whitelist_encode_host: the same plus sct_encode_var on the lines, host pointers;
 * call with max_lines = 0 to learn nlines and max_len, then with room for nlines. */
int sct_lines(const uint8_t* d_buf, int64_t nbytes, int64_t max_lines, int64_t* d_starts, int32_t* d_lens,
              int64_t* nlines, int32_t* max_len, void* stream);
/* sct_whitelist_encode (device, ASYNCHRONOUS on stream: no host synchronisation): the same
 * split, chop and encode: a one-read pass for files of 16-base lines (checked on the fly), else a
 * count pass over the file's tiles and an encode pass that numbers the lines from the tile counts;
 * *d_nlines (int64) and *d_maxlen (int32, the longest chopped line) are written on the device;
 * lines g < min(max_lines, *d_nlines) get d_starts[g], d_lens[g], `words` limbs of d_codes,
 * d_gc[g] (nullable) and d_flags[g] (nullable: bit 0 ambiguous, bit 1 invalid byte, bit 2 too long
 * for `words`); rows g >= max_lines are never written, rows in [*d_nlines, max_lines) are
 * unspecified. */
int sct_whitelist_encode(const uint8_t* d_buf, int64_t nbytes, int kind, int words, int64_t max_lines,
                         uint64_t* d_codes, int64_t* d_starts, int32_t* d_lens, uint8_t* d_gc, uint8_t* d_flags,
                         int64_t* d_nlines, int32_t* d_maxlen, void* stream);
int sct_whitelist_encode_host(const uint8_t* buf, int64_t nbytes, int kind, int words, int64_t max_lines,
                              int64_t* nlines, int32_t* max_len, uint64_t* codes, int64_t* starts,
                              int32_t* lens, uint8_t* flags);

/* ---------------------------------------------------------------- decoders
 * TwoBit(L).decode (encodings.py:90-100): exactly L bytes from the LSB upward,
 * bits above 2L ignored.  out: n*L bytes.
 */
int sct_decode2(const uint64_t* codes, int64_t n, int words, int L, uint8_t* out, void* stream);
int sct_decode2_host(const uint64_t* codes, int64_t n, int words, int L, uint8_t* out);
/* ThreeBit.decode (encodings.py:169-180): bytes up to the highest non-zero triplet.
 * out: n*maxlen bytes, record r's sequence right-aligned in its maxlen slot
 * (so it ends at out[(r+1)*maxlen-1]); lengths[r] = its length;
 * bad[r] = -1, or the value (0, 5 or 7) of the lowest-order triplet below the top
 * non-zero one that has no decoding (the reference raises KeyError(value)).
 * maxlen must be >= ceil(64*words/3).
 */
int sct_decode3(const uint64_t* codes, int64_t n, int words, int maxlen, uint8_t* out,
                int32_t* lengths, int32_t* bad, void* stream);
int sct_decode3_host(const uint64_t* codes, int64_t n, int words, int maxlen, uint8_t* out,
                     int32_t* lengths, int32_t* bad);

/* ---------------------------------------------------------------- gc_content
 * TwoBit(L).gc_content (encodings.py:102-111): low bit of each of the L 2-bit groups.
 * ThreeBit.gc_content  (encodings.py:182-192): bit 0 of every triplet of the code.
 * kind 2 uses L; kind 3 ignores it.  out: n int32.
 */
int sct_gc_content(int kind, const uint64_t* codes, int64_t n, int words, int L, int32_t* out,
                   void* stream);
int sct_gc_content_host(int kind, const uint64_t* codes, int64_t n, int words, int L, int32_t* out);

/* ---------------------------------------------------------------- element-wise Hamming
 * TwoBit.hamming_distance (encodings.py:113-121) / ThreeBit.hamming_distance
 * (encodings.py:194-202) of a[r] vs b[r]: number of non-zero 2-bit (3-bit) groups
 * of a^b.  out: n int32.
 */
int sct_hamming_pairs(int kind, const uint64_t* a, const uint64_t* b, int64_t n, int words,
                      int32_t* out, void* stream);
int sct_hamming_pairs_host(int kind, const uint64_t* a, const uint64_t* b, int64_t n, int words,
                           int32_t* out);

/* ---------------------------------------------------------------- scalar server
 * The *_host calls above with n <= 64 records (the drop-in's scalar methods, e.g.
 * TwoBit.encode / hamming_distance, encodings.py:75-121) are served by a resident
 * one-wave kernel per host thread and device that polls a page-locked mailbox, instead of
 * one kernel launch per call; it exits by itself after SCT_TUNE_SCALAR_IDLE_MS (default 5) idle
 * milliseconds and before any kernel that sizes its grid to the resident workgroups.
 * sct_tune_set(SCT_TUNE_SCALAR_SERVER, 0) turns it off (every call is then a launch).
 * sct_scalar_server_stop: ask every server of the process to exit and wait for it.
 * sct_scalar_server_status: server launches so far and servers running now (either may
 * be NULL).
 */
int sct_scalar_server_stop(void);
int sct_scalar_server_status(int64_t* launches, int* running);

/* ---------------------------------------------------------------- all-pairs histogram
 * Replaces the pair loop of Barcodes.summarize_hamming_distances
 * (src/sctools/barcode.py:42-43: itertools.combinations + TwoBit.hamming_distance).
 *
 * A plan holds the bit-sliced selection table of n device-resident uint64 codes
 * (the TwoBit distance is taken over the low `code_bits` bits, code_bits in
 * [1, 64]; every code must be < 2^code_bits).  The unordered pairs i<j are cut
 * into `items` equal work items (row block x column chunk) so that callers can
 * shard them: any partition of [0, items) into ranges, counted on any number of
 * devices and summed, gives the same result.
 *
 * Two count schemes (a plan has one, fixed at creation):
 *
 * SCT_ALLPAIRS_SUBSETS (any code width): sct_allpairs_count ACCUMULATES (atomic add)
 *   ncounts = nbins uint64 "subset counts" into d_counts: d_counts[0] += pairs counted,
 *   d_counts[m] += #pairs whose distance d has all bits of m set (d & m == m),
 *   m = 1..nbins-1.  Every item range is self-contained: its counts invert alone.
 *
 * SCT_ALLPAIRS_MOMENTS (codes of 29..32 bits = 16 bases, the 10x barcode width): the
 *   count kernel accumulates d_counts[0] += pairs and d_counts[1+i] += #pairs whose
 *   d mod 16 has all bits of kMomProducts[i] set (13 products, sct_common.h), and
 *   sct_allpairs_moments accumulates d_counts[14+k-1] += M_k = sum over ALL pairs of
 *   C(16 - d, k), k = 1..3 (pairs agreeing on k chosen positions, from the codes'
 *   position marginals).  ncounts = 17; only the counts of the WHOLE job (every item
 *   counted once, every moment part added once) invert.  13 products instead of 16
 *   cut the count kernel's VALU work per pair.
 *
 * SCT_ALLPAIRS_SPECTRAL (the same 16-base codes): no pair is enumerated.  The histogram
 *   comes from the Walsh-Hadamard transform F of the codes' multiplicity f over Z_2^32:
 *   S_w = sum of F(z)^2 over the z with w non-zero 2-bit digits, w = 0..16, accumulated as
 *   three limbs that never carry (a multiset's sum_w S_w = 2^32 sum f^2 may exceed 2^64):
 *   d_counts[2+w] += bits 0..31, d_counts[19+w] += bits 32..63, d_counts[36+w] += bits 64..
 *   of every partial sum, so S_w = c[2+w] + 2^32 c[19+w] + 2^64 c[36+w]; d_counts[0] += n and
 *   d_counts[1] += sum f^2 (computed from the sorted codes) once, by the range holding item
 *   0.  ncounts = 53.  The host checks S_0 = n^2 and sum_w S_w = 2^32 sum f^2 exactly.
 *   The items are the 2^18 transform slices (z >> 14); the cost of a slice does not
 *   depend on n, so AUTO picks this scheme for large whitelists.  Only
 *   the counts of the whole job invert (host: Krawtchouk transform, checked exact).
 *
 * The counts are linear, so they may be summed across devices (RCCL all-reduce)
 * before sct_counts_to_hist_ex.
 */
typedef struct sct_allpairs_plan sct_allpairs_plan;

#define SCT_ALLPAIRS_AUTO (-1)    /* 16 bases: SPECTRAL from 325K codes, else MOMENTS; else SUBSETS */
#define SCT_ALLPAIRS_SUBSETS 0
#define SCT_ALLPAIRS_MOMENTS 1
#define SCT_ALLPAIRS_SPECTRAL 2

/* Plan flags (sct_allpairs_plan_create_ex2):
 * SCT_ALLPAIRS_DISTINCT  the caller promises pairwise-distinct codes (the keys of a mapping, as
 *   Barcodes.summarize_hamming_distances has them, barcode.py:39-46), so SPECTRAL takes
 *   sum f^2 = n instead of sorting the codes; a broken promise fails the host's exact check
 *   (SCT_E_RANGE), it never yields a histogram. */
#define SCT_ALLPAIRS_DISTINCT 1
/* SCT_ALLPAIRS_NO_CACHE  the plan allocates its own device buffers and frees them when destroyed,
 *   instead of borrowing its device's cached workspace (see sct_allpairs_cache_release). */
#define SCT_ALLPAIRS_NO_CACHE 2

/* = sct_allpairs_plan_create_ex(..., SCT_ALLPAIRS_AUTO, plan) */
int sct_allpairs_plan_create(const uint64_t* d_codes, int64_t n, int code_bits,
                             sct_allpairs_plan** plan);
int sct_allpairs_plan_create_ex(const uint64_t* d_codes, int64_t n, int code_bits, int scheme,
                                sct_allpairs_plan** plan);
/* = sct_allpairs_plan_create_ex with SCT_ALLPAIRS_* flags */
int sct_allpairs_plan_create_ex2(const uint64_t* d_codes, int64_t n, int code_bits, int scheme, int flags,
                                 sct_allpairs_plan** plan);
int sct_allpairs_plan_destroy(sct_allpairs_plan* plan);
/* nbins = max distance + 1 = 2*ceil(code_bits/4)+1; items = number of work items */
int sct_allpairs_plan_info(const sct_allpairs_plan* plan, int* nbins, int64_t* items,
                           int64_t* pairs);
/* scheme of the plan, length of its counts vector, and its code width */
int sct_allpairs_plan_scheme(const sct_allpairs_plan* plan, int* scheme, int* ncounts,
                             int* code_bits);
/* (Re)build the selection table from the codes the plan was created on. */
int sct_allpairs_build(sct_allpairs_plan* plan, void* stream);
/* Build only what counting items [item_begin, item_end) reads (its column chunks; the
 * MOMENTS scheme also re-sorts the codes): a rank of a sharded job calls this with its
 * own item range. */
int sct_allpairs_build_items(sct_allpairs_plan* plan, int64_t item_begin, int64_t item_end,
                             void* stream);
/* Count work items [item_begin, item_end).  grid = 0 picks the persistent grid size. */
int sct_allpairs_count(sct_allpairs_plan* plan, int64_t item_begin, int64_t item_end,
                       uint64_t* d_counts, int grid, void* stream);
/* MOMENTS scheme: add part `part` of `nparts` of the agreement moments to d_counts
 * (the position subsets are split into nparts shares; summing every part once gives
 * M_1..M_3).  SUBSETS scheme: no-op. */
int sct_allpairs_moments(sct_allpairs_plan* plan, int part, int nparts, uint64_t* d_counts,
                         void* stream);
/* Host-only (no device needed): the plan geometry for n codes of code_bits bits, i.e.
 * what sct_allpairs_plan_info would report, plus rows per item and codes per column
 * chunk.  Lets shard drivers partition [0, items) before touching a GPU. */
int sct_allpairs_geometry(int64_t n, int code_bits, int* nbins, int64_t* items, int* rows_per_item,
                          int* cols_per_item);
/* Pairs contained in work items [item_begin, item_end) (host arithmetic; SPECTRAL: the
 * range's share floor(P*end/items) - floor(P*begin/items) of all P pairs). */
int sct_allpairs_range_pairs(const sct_allpairs_plan* plan, int64_t item_begin, int64_t item_end,
                             int64_t* pairs);

/* Close pairs of a SUBSETS plan (its table keeps the caller's order; MOMENTS and SPECTRAL plans:
 * SCT_E_INVALID).
 * Every unordered pair i<j of the plan's codes in items [item_begin, item_end) with
 * TwoBit distance <= max_d (0..3; else SCT_E_RANGE).  n < 2^31 and room < 2^31 (else SCT_E_RANGE).
 * The call overwrites all its outputs:
 *   d_stats (6 uint64): [0] pairs found, [1] pairs stored = min(found, room), [2+d] pairs at distance d;
 *   d_i, d_j, d_dist (room entries; nullable when room == 0): the stored pairs.  When found <= room
 *     they are all of them, ascending by (i, j); when found > room WHICH pairs are stored is
 *     unspecified, each is a true close pair and none repeats, and nothing past `room` is written;
 *   d_degree (nullable; n * (max_d+1) uint32): [k*(max_d+1)+d] = positions at distance d from k
 *     among the pairs of this item range (both ends counted; exact whatever `room`).
 * Results of disjoint item ranges concatenate (pairs) and add (stats, degree).
 * May wait on `stream` (the sort needs the count).  Needs a built plan. */
int sct_allpairs_close_pairs(sct_allpairs_plan* plan, int64_t item_begin, int64_t item_end, int max_d,
                             int32_t* d_i, int32_t* d_j, uint8_t* d_dist, int64_t room,
                             uint64_t* d_stats, uint32_t* d_degree, void* stream);
/* One-shot, host pointers, current device: the same over all pairs of the n codes (a SUBSETS plan of
 * the call's own, built, run over every item and destroyed).  n < 2: no pairs, SCT_OK. */
int sct_close_pairs_host(const uint64_t* codes, int64_t n, int code_bits, int max_d,
                         int32_t* i, int32_t* j, uint8_t* dist, int64_t room,
                         uint64_t* stats, uint32_t* degree);

/* Bench aid (d_counts receives garbage): the dominant kernel's ms per launch, timed as
 * `repeats` back-to-back launches bracketed by HIP events on `stream`.  SPECTRAL: out[0] =
 * tile kernel, out[1] = seed kernel, both on the first chunk of the range (out[2] = its
 * slices); other schemes: out[0] = count kernel over the range, out[1] = 0, out[2] = items.
 * Needs a built plan. */
int sct_allpairs_time_kernels(sct_allpairs_plan* plan, int64_t item_begin, int64_t item_end,
                              uint64_t* d_counts, int repeats, double* out, void* stream);

/* Test aid: the seed values of slices [slice_begin, slice_end) of a built SPECTRAL plan with int8
 * seeds on 14-bit columns, by the seed kernel sct_allpairs_count would launch, into d_out:
 * d_out[(z - slice_begin) * 16384 + c] for slice z and column c, (slice_end - slice_begin) * 16384
 * bytes.  Plans with other seeds: SCT_E_INVALID. */
int sct_allpairs_seed_slices(sct_allpairs_plan* plan, int64_t slice_begin, int64_t slice_end, int8_t* d_out,
                             void* stream);
/* Test aid: the seed rows of slices [slice_begin, slice_end) of a built SPECTRAL plan, whatever its
 * seed, exactly as the tile kernel reads them, by the seed kernel and grid sct_allpairs_count would
 * launch for that range.  The slices are the transform's real slices: 2^18 on 14-bit columns, 2^16
 * on 16-bit columns (sct_allpairs_spectral_columns).  A row is 2^column_bits values of elem_bytes
 * (sct_allpairs_spectral_info) bytes, little-endian signed: the row of slice z starts at d_out +
 * (z - slice_begin) * 2^column_bits * elem_bytes.  int8 rows hold column c at position c.  int16
 * and int32 rows (14-bit columns) hold it at position pos(c), so that one 16-byte chunk carries
 * V = 16 / elem_bytes columns of one tile thread (L = log2 V):
 *   pos(c) = (c & (V-1)) | (((c >> 4) & 255) << L) | (((c >> L) & (16/V - 1)) << (L + 8)) | ((c >> 12) << 12)
 * i.e. the column's low L bits, then its bits 4..11, then its bits L..3, then its bits 12, 13.
 * out_bytes must equal (slice_end - slice_begin) * row bytes.  SCT_E_INVALID, and nothing is
 * written: a plan that is not SPECTRAL or holds fewer than 2 codes, an empty range or one outside
 * the plan's slices, any other out_bytes. */
int sct_allpairs_seed_rows(sct_allpairs_plan* plan, int64_t slice_begin, int64_t slice_end, void* d_out,
                           int64_t out_bytes, void* stream);

/* SPECTRAL plans: bytes per seed value of the seed -> tile intermediate (1, 2 or 4: the
 * densest transform column bounds it), slices per seed / tile launch, codes in the densest
 * column.  Other schemes: SCT_E_INVALID. */
int sct_allpairs_spectral_info(const sct_allpairs_plan* plan, int* elem_bytes, int64_t* chunk_slices,
                               int* max_column);
/* SPECTRAL plans: the transform's column width, 14 (2^18 slices of 2^14 columns) or 16 for sets
 * whose densest 14-bit column needs int16 seeds but whose densest 16-bit column holds <= 127
 * codes (2^16 slices of 2^16 columns, int8 seeds; items stay 2^18 virtual slices, 4 per real
 * slice).  Replaces nothing in the reference (an internal layout choice). */
int sct_allpairs_spectral_columns(const sct_allpairs_plan* plan, int* column_bits);

/* Bench aid: per-launch HIP-event timing of this plan's kernels, recorded on the stream each
 * launch runs on (so it times the launches of a real run, pipelined or not).  mode 1 = start
 * (zeroes the sums), 0 = stop, 2 = read and keep recording.  out (nullable, 8 doubles) =
 * [ms, launches] summed over the recorded launches of kind 0 seed, 1 tile (SPECTRAL), 2 pair
 * count kernel (SUBSETS / MOMENTS), 3 table build (one span per build call); the call waits
 * for the recorded launches. */
int sct_allpairs_timing(sct_allpairs_plan* plan, int mode, double* out);

/* Host: SUBSETS counts -> histogram (exact Moebius inversion), hist[d] for d < nbins. */
int sct_counts_to_hist(const uint64_t* counts, int nbins, uint64_t* hist);
/* Host: counts of any scheme -> histogram (MOMENTS: exact rational solve of the
 * 17 x 17 system; SPECTRAL: Krawtchouk transform; both checked integral and
 * non-negative).  nbins must be the plan's. */
int sct_counts_to_hist_ex(int scheme, const uint64_t* counts, int ncounts, uint64_t* hist,
                          int nbins);

/* One-shot, host pointers, current device: histogram of TwoBit distances over all
 * unordered pairs of the n codes.  hist must hold nbins = 2*ceil(code_bits/4)+1. */
int sct_hamming_hist_allpairs_host(const uint64_t* codes, int64_t n, int code_bits,
                                   uint64_t* hist, int nbins);
/* the same with SCT_ALLPAIRS_DISTINCT.  By default a one-shot call leaves no device memory
 * behind: its plan and staging buffers are its own and freed before it returns (4 GiB for a
 * 16-base set from 325K codes).  sct_keep_workspace(1) keeps them cached per device instead, so
 * repeated calls map nothing (previous: the setting before the call; keep < 0 only reads it). */
int sct_hamming_hist_allpairs_host_ex(const uint64_t* codes, int64_t n, int code_bits, int flags,
                                      uint64_t* hist, int nbins);
int sct_keep_workspace(int keep, int* previous);

/* ---------------------------------------------------------------- several devices, one process
 * SURVEY §8(b) `n_gpus` (sct_init(n_gpus) / an n_gpus argument in the survey's sketch): the
 * one-shot and host-stream calls split across devices[0..ndev) of this process (HIP ordinals;
 * repeats are logical shards of one GPU).  Slot r runs on a persistent worker thread of its own
 * with devices[r] current; the calling thread's current device is not changed.  devices == NULL
 * or ndev == 1: the single-device call on the current device (or devices[0]).  One multi-device
 * call runs at a time per process (calls from several threads queue).
 *
 * All-pairs (replaces barcode.py:42-43 like sct_hamming_hist_allpairs_host_ex): every slot holds
 * a replica of the codes and counts the item range items*r/ndev .. items*(r+1)/ndev (SPECTRAL:
 * transform slices) plus moment part r of ndev; the 53 / 17 / nbins counts of the slots are summed
 * on the host -- where they are needed anyway -- and inverted once.  Bit-identical for any ndev. */
int sct_hamming_hist_allpairs_host_devices(const uint64_t* codes, int64_t n, int code_bits, int flags,
                                           const int* devices, int ndev, uint64_t* hist, int nbins);
/* Nearest whitelist: contiguous query ranges per slot, the whitelist indexed on every device
 * (no exchange).  The multi plan keeps one index per slot for a stream of query batches. */
int sct_nearest_host_devices(int kind, const uint64_t* whitelist, int64_t nw, const uint64_t* queries, int64_t nq,
                             int code_bits, int max_d, const int* devices, int ndev, int32_t* index,
                             uint8_t* dist);
typedef struct sct_nearest_multi sct_nearest_multi;
int sct_nearest_multi_create_host(int kind, const uint64_t* whitelist, int64_t nw, int code_bits, int max_d,
                                  const int* devices, int ndev, sct_nearest_multi** plan);
int sct_nearest_multi_query_host(sct_nearest_multi* plan, const uint64_t* queries, int64_t nq, int32_t* index,
                                 uint8_t* dist);
/* sct_nearest_count_host over the same split: every slot tallies into a host array of its own and
 * the arrays are summed into counts / tally after the slots return. */
int sct_nearest_multi_count_host(sct_nearest_multi* plan, const uint64_t* queries, int64_t nq, uint64_t* counts,
                                 uint64_t* tally);
/* sct_nearest_plan_set_posterior_host / sct_nearest_correct_host / sct_nearest_correct_count_host over
 * the same split: the prior is replicated (every slot permutes it for its own index), queries and
 * quality rows go to the slots as contiguous ranges, and the slots' statistics are summed. */
int sct_nearest_multi_set_posterior_host(sct_nearest_multi* plan, const uint32_t* prior, const uint32_t* qweight,
                                         int num, int den);
int sct_nearest_multi_correct_host(sct_nearest_multi* plan, const uint64_t* queries, const uint8_t* qual,
                                   int64_t qual_stride, int64_t nq, int32_t* index, uint8_t* dist, uint64_t* stats);
int sct_nearest_multi_correct_count_host(sct_nearest_multi* plan, const uint64_t* queries, const uint8_t* qual,
                                         int64_t qual_stride, int64_t nq, uint64_t* counts, uint64_t* tally,
                                         uint64_t* stats);
int sct_nearest_multi_destroy(sct_nearest_multi* plan);
/* Host encode stream (sct_encode_stream_host) over contiguous record ranges, one per slot. */
int sct_encode_stream_host_devices(int kind, const uint8_t* seqs, int64_t n, int L, uint64_t* codes, uint8_t* gc,
                                   uint8_t* flags, int64_t chunk, const int* devices, int ndev);

/* Plan cache: a plan created while no other plan holds its device's cached buffers borrows
 * them (the SPECTRAL intermediate of up to 4 GiB, codes, bit planes, order table) and leaves
 * them allocated when destroyed, so repeated one-shot calls map no device memory (the
 * drop-in's summarize_hamming_distances, barcode.py:39-46, is one such call).  This frees
 * every idle cache (all devices); a cache lent to a live plan is freed when that plan is
 * destroyed.  sct_tune_set(SCT_TUNE_PLAN_CACHE, 0) turns the cache off.  The idle memory of
 * the library's stream-ordered scratch pool (host-stream stages, ingest scratch) is trimmed
 * too, after a synchronisation of the current device, and the calling thread's staging buffer
 * on the current device is freed. */
int sct_allpairs_cache_release(void);

/* ---------------------------------------------------------------- all-pairs, wide codes
 * The same pair loop (barcode.py:42-43) for keys of any width up to 256 limbs: codes are
 * n x `words` little-endian uint64 limbs (Python ints >= 2^64: ThreeBit-encoded 22..28-bp
 * barcodes, TwoBit > 32 bp).  TwoBit.hamming_distance (encodings.py:113-121) of multi-limb
 * codes = the sum of the per-limb counts (no 2-bit group straddles a limb).  Work items
 * are pairs of 256-code tiles (a <= b, row-major), so contiguous item ranges shard across
 * devices; sct_allpairs_wide ACCUMULATES hist[d] (nbins = 32 * words + 1 uint64) with
 * the pairs i < j of items [item_begin, item_end). */
int sct_allpairs_wide_geometry(int64_t n, int words, int64_t* items, int* nbins);
int sct_allpairs_wide_range_pairs(int64_t n, int64_t item_begin, int64_t item_end, int64_t* pairs);
int sct_allpairs_wide(const uint64_t* d_codes, int64_t n, int words, int64_t item_begin, int64_t item_end,
                      uint64_t* d_hist, int nbins, void* stream);
int sct_hamming_hist_allpairs_wide_host(const uint64_t* codes, int64_t n, int words, uint64_t* hist,
                                        int nbins);

/* ---------------------------------------------------------------- base frequency
 * Replaces Barcodes.base_frequency (src/sctools/barcode.py:48-70): out[p*4 + v] =
 * number of codes whose base p (0 = first, MSB-first TwoBit packing) has 2-bit value
 * v (A 0, C 1, T 2, G 3); bases above bit 63 read as 0, as the reference's uint64
 * keys >>= 2 loop does.  out: L*4 uint64, overwritten.  L <= 1024.
 */
int sct_base_frequency(const uint64_t* codes, int64_t n, int L, uint64_t* out, void* stream);
int sct_base_frequency_host(const uint64_t* codes, int64_t n, int L, uint64_t* out);

/* ---------------------------------------------------------------- nearest whitelist
 * No reference function exists; the contract is the brute-force
 * composition of the reference's distance (kind 2: TwoBit.hamming_distance,
 * encodings.py:113-121; kind 3: ThreeBit.hamming_distance, encodings.py:194-202):
 *   index[i] = j  if exactly one whitelist index j attains d_min(q_i) <= max_d,
 *            = -2 if several indices attain it, -1 if d_min > max_d;
 *   dist[i]  = d_min if <= max_d, else 255.
 * The plan is an exact pigeonhole index (max_d <= 1 on A/C/G/T whitelists: half-key tables;
 * otherwise open-addressing or CSR buckets per position block); it copies nothing from the
 * caller after create returns (the whitelist is bucketed).  A half-key whitelist sorted
 * alphabetically, or numerically as TwoBit or ThreeBit codes, is queried in one kernel (table
 * position = whitelist index); any other order adds a pass mapping positions to indices.  The
 * answers never depend on the order.
 * code_bits: bits covered by the block split (whitelist codes < 2^code_bits).
 */
typedef struct sct_nearest_plan sct_nearest_plan;
int sct_nearest_plan_create(int kind, const uint64_t* d_whitelist, int64_t nw, int code_bits,
                            int max_d, void* stream, sct_nearest_plan** plan);
int sct_nearest_plan_destroy(sct_nearest_plan* plan);
int sct_nearest_query(sct_nearest_plan* plan, const uint64_t* d_queries, int64_t nq,
                      int32_t* d_index, uint8_t* d_dist, void* stream);
/* the index layout the plan chose and its device bytes */
#define SCT_NEAREST_OA 1       /* open-addressing tables of block-pair keys */
#define SCT_NEAREST_CSR 2      /* CSR buckets per block */
#define SCT_NEAREST_HALVES 3   /* sorted half-key tables (max_d <= 1, ACGT whitelists) */
int sct_nearest_plan_info(const sct_nearest_plan* plan, int* scheme, int64_t* index_bytes);
int sct_nearest_host(int kind, const uint64_t* whitelist, int64_t nw, const uint64_t* queries,
                     int64_t nq, int code_bits, int max_d, int32_t* index, uint8_t* dist);
/* A plan from a HOST whitelist (copied for the build, not kept), and queries from host memory
 * against it: a stream of batches builds the index once (barcode.WhitelistCorrector).  The
 * query call copies the queries in, runs sct_nearest_query on the thread's stream with scratch
 * from the library's stream-ordered pool, and returns with index / dist in host memory
 * (page-locked buffers are copied by DMA in place). */
int sct_nearest_plan_create_host(int kind, const uint64_t* whitelist, int64_t nw, int code_bits, int max_d,
                                 sct_nearest_plan** plan);
int sct_nearest_query_host(sct_nearest_plan* plan, const uint64_t* queries, int64_t nq, int32_t* index,
                           uint8_t* dist);

/* Posterior correction of the queries sct_nearest_query gives up on: those with several whitelist
 * barcodes at distance 1 (-2 there), resolved by base quality and whitelist priors as single-cell
 * pipelines do.  No reference function exists; the distance d is the
 * reference's (kind 2: TwoBit.hamming_distance, encodings.py:113-121; kind 3:
 * ThreeBit.hamming_distance, encodings.py:194-202), over ALL whitelist indices (a duplicated code is
 * two indices), and everything is integer arithmetic.  With L = the plan's positions
 * (ceil(code_bits / kind)), for query q with quality row qual (L raw bytes; byte b belongs to base
 * b, the first base, which is digit L - 1 - b of the code):
 *   1. q has a bit at or above kind * L:            index -1, dist 255;
 *   2. some index has d == 0:                       that index if it is the only one, else -2; dist 0;
 *   3. candidates = every j with d(q, w_j) == 1 and prior[j] > 0, p_j the one base where they differ
 *      (an N or an invalid ThreeBit triplet of the query is such a base),
 *      score_j = prior[j] * qweight[qual[p_j]] (uint64);
 *   4. no candidate:                                index -1, dist 255;
 *   5. best = the largest score, total = their sum: index = its j if den * best >= num * total,
 *      else -2; dist 1.
 * prior: nw uint32 values < 2^30 (NULL: all ones); qweight: 256 HOST values in [1, 2^20] indexed by
 * the raw quality byte; 1 <= num <= den <= 64 and 2 * num > den (the winner is unique); anything
 * else is SCT_E_INVALID.  So a score is < 2^50, a total of at most 48 < 2^56, and den * total < 2^62.
 * Only half-key plans qualify (kind 2 or 3, max_d == 1, an A/C/G/T whitelist of 2..16 positions):
 * any other plan is SCT_E_RANGE.  set_posterior may be called again at any time (it waits for the
 * plan's calls in flight and for `stream`); it holds for the calls after it.
 * sct_nearest_correct is asynchronous on `stream`: the query pass appends the queries of case 3 to a
 * device worklist instead of answering -2 (with a prior set, those with one candidate too), and a
 * second kernel scores only those, so only their quality rows (qual_stride >= L bytes apart) are
 * read.  d_stats (nullable, 2 uint64, ACCUMULATED): [0] queries scored, [1] those given an index.
 * The host forms copy queries and rows in (rows packed to L bytes) and index / dist, or only the
 * counts and tallies of sct_index_tally, out; stats (nullable) is accumulated there as well. */
int sct_nearest_plan_set_posterior(sct_nearest_plan* plan, const uint32_t* d_prior, const uint32_t* qweight,
                                   int num, int den, void* stream);
int sct_nearest_plan_set_posterior_host(sct_nearest_plan* plan, const uint32_t* prior, const uint32_t* qweight,
                                        int num, int den);
int sct_nearest_correct(sct_nearest_plan* plan, const uint64_t* d_queries, const uint8_t* d_qual,
                        int64_t qual_stride, int64_t nq, int32_t* d_index, uint8_t* d_dist, uint64_t* d_stats,
                        void* stream);
int sct_nearest_correct_host(sct_nearest_plan* plan, const uint64_t* queries, const uint8_t* qual,
                             int64_t qual_stride, int64_t nq, int32_t* index, uint8_t* dist, uint64_t* stats);
int sct_nearest_correct_count_host(sct_nearest_plan* plan, const uint64_t* queries, const uint8_t* qual,
                                   int64_t qual_stride, int64_t nq, uint64_t* counts, uint64_t* tally,
                                   uint64_t* stats);

/* ---------------------------------------------------------------- counting observed barcodes
 * Replaces the host Counter of Barcodes.from_iterable_encoded (src/sctools/barcode.py:100-102,
 * `Counter(iterable)`) for codes below 2^64: a streaming device group-by with Counter's semantics.
 * Per distinct code the counter keeps its count and the global position (over every update so far)
 * of its first occurrence; fetch returns the rows ordered by that position, which is Counter's
 * iteration order, whatever order the device counted in.
 * The table is open addressing with 64-bit atomics (claim by compare-and-swap, bounded probes) and
 * grows by itself: capacity_hint only sizes the first table (rounded up to a power of two, >= 64).
 * Every code is legal, 2^64 - 1 (the table's empty mark) included.  update feeds sub-batches and
 * reads the table's size between them when it may have to grow, so it is asynchronous on `stream`
 * only while the table has room; a call on another stream waits for the counter's earlier work.
 * info: nunique = distinct codes, total = codes seen, capacity = table slots (each nullable).
 * fetch: keys / counts / first of the nunique rows; room < nunique is SCT_E_INVALID and leaves the
 * counter as it was.  A table that fills up in spite of the growth rule is SCT_E_RANGE.
 * destroy waits for the work the counter enqueued. */
typedef struct sct_counter sct_counter;
int sct_counter_create(int64_t capacity_hint, sct_counter** counter);
int sct_counter_update(sct_counter* counter, const uint64_t* d_codes, int64_t n, void* stream);
int sct_counter_update_host(sct_counter* counter, const uint64_t* codes, int64_t n);
int sct_counter_info(sct_counter* counter, int64_t* nunique, int64_t* total, int64_t* capacity);
int sct_counter_fetch_host(sct_counter* counter, uint64_t* keys, uint64_t* counts, int64_t* first, int64_t room);
int sct_counter_fetch(sct_counter* counter, uint64_t* d_keys, uint64_t* d_counts, int64_t* d_first, int64_t room,
                      void* stream);
int sct_counter_destroy(sct_counter* counter);
/* Reads per whitelist barcode (no reference function; the host form is np.bincount over
 * sct_nearest_query's index): d_counts[j] += 1 for every index j in [0, nw), d_tally[0] += 1 for
 * every -1 (no match) and d_tally[1] += 1 for every -2 (tie); d_counts: nw uint64, d_tally: 2 uint64,
 * both ACCUMULATED.  An index outside [-2, nw) is not counted and makes the call SCT_E_RANGE; the
 * call waits for the stream to learn that.
 * sct_nearest_count_host: the queries in, sct_nearest_query and the tally on the thread's stream
 * with pool scratch, and only nw counts + 2 tallies back, ADDED to the caller's host arrays (what
 * sct_nearest_query_host returns is 5 bytes per query).  nq == 0 changes nothing. */
int sct_index_tally(const int32_t* d_index, int64_t n, int64_t nw, uint64_t* d_counts, uint64_t* d_tally,
                    void* stream);
int sct_nearest_count_host(sct_nearest_plan* plan, const uint64_t* queries, int64_t nq, uint64_t* counts,
                           uint64_t* tally);

/* Counting molecules: distinct (corrected barcode, UMI) pairs per whitelist barcode, which removes
 * PCR duplicates.  No reference function exists (the reference extracts the UMI, fastq.py:181-200,
 * and counts nothing with it); the contract is the one below, restated in plain Python by
 * tests/molecules_reference.py.
 * A counter is created for nw whitelist barcodes (1 <= nw < 2^31), a UMI encoding kind (2 TwoBit,
 * 3 ThreeBit) and a UMI length L.  With umi_bits = kind * L and idx_bits = max(1, bit_length(nw - 1)),
 * 1 <= umi_bits and idx_bits + umi_bits <= 63 are required (else SCT_E_INVALID).  A molecule's key is
 * (index << umi_bits) | umi; its top bit is always 0, so the table's empty mark 2^64 - 1 is never
 * a key and no side slot is needed.  For read i of an update, with index[i] as sct_nearest_query /
 * sct_nearest_correct leave it and umi[i] the UMI's code:
 *   1. index == -1:                  tally[0] += 1 (no match);
 *   2. index == -2:                  tally[1] += 1 (ambiguous);
 *   3. index outside [-2, nw):       not counted, nothing is stored through it, and the call is
 *                                    SCT_E_RANGE; the rest of the batch is counted (sct_index_tally's rule);
 *   4. index >= 0 and a bad UMI:     tally[2] += 1 and the read counts nowhere else.  A UMI is bad if it
 *                                    has a bit at or above umi_bits, or (kind 3) if any of its L triplets
 *                                    is not C 1, A 2, G 3 or T 4: N = 6, the invalid 0 / 5 / 7, and a
 *                                    zero leading triplet.  For kind 2 every value below 2^umi_bits is good;
 *   5. otherwise                     reads[index] += 1, and molecules[index] += 1 if the key has not been
 *                                    seen in this counter's lifetime.
 * reads[nw], molecules[nw] (uint64) and tally[3] live on the device with the counter, are zeroed at
 * create and accumulate over every update; everything is exact integers.
 * The table holds keys only (8 B per slot), claimed by a 64-bit compare-and-swap with bounded probes
 * as the counter's is, and grows by the counter's rule: capacity_hint sizes the first table (a power
 * of two >= 64), 2^31 slots at most; a table that fills up all the same is SCT_E_RANGE.  update
 * enqueues its sub-batches on `stream` (reading the table's size between them only when it may have
 * to grow, as sct_counter_update does) and then waits for the stream once, as sct_index_tally does,
 * to learn of an out-of-range index (rule 3): it returns after the batch's kernels.  A call on
 * another stream waits for the counter's earlier work.  n == 0 changes nothing and needs no pointer.
 * info: nmolecules = distinct keys, total = reads fed whatever became of them, capacity = table
 * slots (each nullable).  counts: nw + nw + 3 words out, each array nullable.  fetch: the distinct
 * molecules in ascending key order (by barcode index, then by UMI code); room < nmolecules is
 * SCT_E_INVALID and leaves the counter as it was.  The counter lives on the device current at
 * create (create_ex: on the device it names); destroy waits for the work the counter enqueued, and
 * destroy(NULL) is SCT_OK.
 * create_ex is the one constructor: flags bit 0 (SCT_MOLECULES_COUNTED) makes a counted counter
 * (below), any other bit is SCT_E_INVALID; device is a HIP ordinal, or -1 for the current device (an
 * ordinal that does not exist is SCT_E_INVALID).  sct_molecules_create is create_ex(.., 0, -1, ..)
 * and sct_molecules_create_counted is create_ex(.., SCT_MOLECULES_COUNTED, -1, ..).
 * Devices: every sct_molecules_* call works whatever device is current and leaves the current device
 * as it found it (the call makes the counter's device current for its own duration).  Device
 * pointers and a non-NULL stream given to a call belong to the counter's device; a NULL stream is
 * that device's default stream. */
#define SCT_MOLECULES_COUNTED 1
typedef struct sct_molecules sct_molecules;
int sct_molecules_create(int64_t nw, int kind, int L, int64_t capacity_hint, sct_molecules** mol);
int sct_molecules_create_ex(int64_t nw, int kind, int L, int64_t capacity_hint, int flags, int device,
                            sct_molecules** mol);
int sct_molecules_update(sct_molecules* mol, const int32_t* d_index, const uint64_t* d_umi, int64_t n, void* stream);
int sct_molecules_update_host(sct_molecules* mol, const int32_t* index, const uint64_t* umi, int64_t n);
int sct_molecules_info(sct_molecules* mol, int64_t* nmolecules, int64_t* total, int64_t* capacity);
int sct_molecules_counts_host(sct_molecules* mol, uint64_t* reads, uint64_t* molecules, uint64_t* tally);
int sct_molecules_counts(sct_molecules* mol, uint64_t* d_reads, uint64_t* d_molecules, uint64_t* d_tally,
                         void* stream);
int sct_molecules_fetch_host(sct_molecules* mol, int32_t* index, uint64_t* umi, int64_t room);
int sct_molecules_fetch(sct_molecules* mol, int32_t* d_index, uint64_t* d_umi, int64_t room, void* stream);
int sct_molecules_destroy(sct_molecules* mol);

/* Collapsing UMIs one base apart: a sequencing error in a UMI base makes one molecule look like two,
 * so a UMI one base away from a better-supported UMI of the same barcode is merged into it before
 * molecules are counted.  The contract is restated in plain Python by tests/umi_collapse_reference.py.
 * A *counted* molecule counter (sct_molecules_create_counted; the same checks as create) is a
 * molecule counter that also keeps mreads[key] for every stored key: the number of rule-5 reads of
 * that molecule over the counter's lifetime, uint64 and exact, in a second array of 8 B per slot
 * beside the keys.  Everything above (rules 1-5, tally, growth, streams, info, counts, fetch) holds
 * for it unchanged; a counter made by sct_molecules_create keeps no such array and runs the code it
 * ran before there were counted ones.
 * Neighbours: N1(umi) is the 3 * L codes that differ from umi in exactly one base position and carry
 * another of the four bases there: for kind 2 a digit d becomes one of the three other values of
 * 0..3, for kind 3 a triplet t of {1, 2, 3, 4} becomes one of the three other values of {1, 2, 3, 4}
 * (N and the invalid triplets are never neighbours).  Index bits never change: the same UMI under
 * two barcodes is unrelated.
 * Parent (one step, evaluated for every molecule against the uncorrected counts): parent(i, u) is
 * the UMI v that maximises the pair (mreads[(i, v)], v), where (a, x) > (b, y) means a > b, or
 * a == b and x > y (the order of the codes, not of the ASCII text), over u itself and the members of
 * N1(u) stored under index i.  A molecule is a root when parent == u.  The rule is not transitive
 * and no read moves twice.
 * collapse describes the state at the call; its results are written, not accumulated:
 *   collapsed[i]  the number of distinct values of parent(i, u) over the molecules (i, u) of barcode
 *                 i -- the images, not the roots.  ThreeBit L = 2 under one barcode, AA x 1, AC x 2,
 *                 GC x 5: parent(AA) = AC, parent(AC) = GC, GC is a root; molecules = 3,
 *                 collapsed = 2 (AC and GC both receive reads), n_corrected = 2, and there is 1 root;
 *   n_corrected   the number of molecules with parent != u (nullable).
 * Reads per barcode do not change (correction never crosses a barcode).  collapse reads the table and
 * mreads only: calling it twice gives the same answer, and later updates are unaffected by it.
 * fetch_counted: exactly fetch's rows in fetch's order, with each row's mreads and, if d_parent is
 * not NULL, its parent's UMI beside them; the room rule is fetch's.  collapse and fetch_counted on a
 * counter that is not counted are SCT_E_INVALID and change nothing.  Both order themselves after
 * the counter's earlier work on other streams, as every call does. */
int sct_molecules_create_counted(int64_t nw, int kind, int L, int64_t capacity_hint, sct_molecules** mol);
int sct_molecules_collapse(sct_molecules* mol, uint64_t* d_collapsed, uint64_t* d_ncorrected, void* stream);
int sct_molecules_collapse_host(sct_molecules* mol, uint64_t* collapsed, uint64_t* ncorrected);
int sct_molecules_fetch_counted(sct_molecules* mol, int32_t* d_index, uint64_t* d_umi, uint64_t* d_mreads,
                                uint64_t* d_parent, int64_t room, void* stream);
int sct_molecules_fetch_counted_host(sct_molecules* mol, int32_t* index, uint64_t* umi, uint64_t* mreads,
                                     uint64_t* parent, int64_t room);

/* Directional clusters: the transitive collapse, UMI-tools' *directional* method, on a counted
 * counter.  The one-step rule above counts images and has no support threshold; here a molecule is
 * merged into whatever reaches it through better-supported UMIs, and the clusters are the molecules.
 * The contract is restated in plain Python by tests/umi_directional_reference.py.
 * Edge: for u, v stored under the same index (and the same feature, on a feature counter: neighbours
 * change UMI bits only) there is an edge u -> v when v is in N1(u) and
 * mreads[u] >= 2 * mreads[v] - 1, evaluated without overflow for any counts >= 1 as
 * mreads[u] >= mreads[v] && mreads[u] - mreads[v] >= mreads[v] - 1.  Two UMIs are joined in both
 * directions exactly when both have 1 read; UMIs with equal reads >= 2 are not joined.
 * Root: order the molecules by (mreads, code), the parent rule's order.  root(v) is the largest
 * molecule, in that order, among v and everything that reaches v along edges; v is a root when
 * root(v) == v, and a cluster is a root with everything whose root it is.
 * This is UMI-tools' sequential procedure -- molecules taken in descending (mreads, code) order, each
 * one not yet claimed becomes a root and claims every unclaimed molecule reachable from it: the
 * largest ancestor w of v has no larger ancestor of its own (that would be an ancestor of v), so
 * nothing claims w before its turn, and v is still unclaimed then because only a larger ancestor
 * could have claimed it.  UMI-tools breaks ties in mreads by insertion order, this contract by code:
 * only the name of the root of mutually joined 1-read UMIs can differ, never the number of clusters,
 * which is the number of strongly connected components with no edge coming in from outside.
 * The entry points below take `method` after the handle: SCT_COLLAPSE_ONE_STEP gives exactly what
 * the entry point without _by gives (which is that call), any value but the two is SCT_E_INVALID,
 * and with SCT_COLLAPSE_DIRECTIONAL
 *   collapse_by        collapsed[i] is the number of roots under barcode i, n_corrected the number of
 *                      molecules with root != self.  ThreeBit L = 2 under one barcode, AA x 1, AC x 2,
 *                      GC x 5: AC -> AA (2 >= 1) and GC -> AC (5 >= 3), so collapsed = 1 and
 *                      n_corrected = 2;
 *   fetch_counted_by,
 *   fetch_features_by  the parent column carries the root's UMI;
 *   matrix_by          collapsed[e] is the number of roots in entry e (a root lies in its cluster's entry).
 * Every other argument, check and result is the sibling's.  The pass reads the table and mreads only:
 * it is repeatable, later updates are unaffected, and it is valid after merge.  On a counter that is
 * not counted it is SCT_E_INVALID and changes nothing.  It orders itself after the counter's earlier
 * work on other streams and checks the overflow word first, as collapse does.  The labels settle in
 * sweeps, one launch each, and the device forms wait for `stream` between them (matrix already waits
 * once); there is no device-side barrier.  More than nmolecules + 2 sweeps is SCT_E_INTERNAL, which
 * correct code never returns.  Scratch: 4 B per slot and 8 B per molecule from the library's pool.
 * directional_info: of the counter's last directional pass, the sweeps, the molecules with an
 * in-edge (the first sweep's worklist) and the molecules all sweeps looked at together (each
 * nullable; a bench aid). */
#define SCT_COLLAPSE_ONE_STEP 0
#define SCT_COLLAPSE_DIRECTIONAL 1
int sct_molecules_collapse_by(sct_molecules* mol, int method, uint64_t* d_collapsed, uint64_t* d_ncorrected,
                              void* stream);
int sct_molecules_collapse_by_host(sct_molecules* mol, int method, uint64_t* collapsed, uint64_t* ncorrected);
int sct_molecules_fetch_counted_by(sct_molecules* mol, int method, int32_t* d_index, uint64_t* d_umi,
                                   uint64_t* d_mreads, uint64_t* d_parent, int64_t room, void* stream);
int sct_molecules_fetch_counted_by_host(sct_molecules* mol, int method, int32_t* index, uint64_t* umi,
                                        uint64_t* mreads, uint64_t* parent, int64_t room);
int sct_molecules_directional_info(sct_molecules* mol, int64_t* sweeps, int64_t* worklist, int64_t* swept);

/* Merging molecule counters: one table from the counters of several files, lanes or devices.  The
 * two reads of a molecule can land in different counters, so molecules[] of two counters cannot be
 * added up: the union of the key sets is taken on the device.
 * After merge(dst, src), dst is the counter that was fed dst's updates followed by src's updates, in
 * every observable respect: info (nmolecules, total), counts (reads, molecules, the three tallies),
 * fetch, fetch_counted (mreads and parent) and collapse -- so collapse is valid across shards.
 * That is: reads[i] += src.reads[i], tally[k] += src.tally[k], total += src.total, every key stored
 * in src is claimed in dst by the update's own rule (molecules[index] += 1 from the lane whose
 * compare-and-swap took the slot, and from no other), and for counted counters mreads of the key in
 * dst += mreads of the key in src.  src is unchanged and stays usable; merging it a second time
 * doubles reads, mreads, the tallies and total and adds no molecule.  The cost is one update pass
 * over src's molecules, not over its reads.
 * Conditions: dst != src, and nw, kind, L and counted-ness equal; a NULL argument or a violated
 * condition is SCT_E_INVALID (the message names what differs).  A src whose table overflowed is
 * SCT_E_RANGE, as fetch treats it.  Growth: before any key moves dst is grown by update's rehash so
 * that dst.nmolecules + src.nmolecules <= capacity / 2 (the smallest such power of two, never less
 * than dst's capacity); more than 2^31 slots is SCT_E_RANGE.  After any of these errors both
 * counters are as they were.  The two sizes are read once (each a wait for the stream); the call is
 * otherwise asynchronous on `stream`, which belongs to dst's device.
 * The merge orders itself after both counters' earlier work on any stream, and the later work of
 * both after itself.  The counters may live on different devices: src's occupied rows are then
 * compacted on its own device and copied into scratch on dst's device (hipMemcpyPeerAsync; peer
 * access is neither needed nor enabled); on one device the kernel reads src's table in place. */
int sct_molecules_merge(sct_molecules* dst, sct_molecules* src, void* stream);

/* Downsampling reads: what the library would have shown at a fraction of its reads -- the saturation
 * curve of a QC report -- and a library thinned to the depth of a shallower one before they are
 * merged (binomial thinning of every molecule's reads).  On counted counters.  The contract is
 * restated in plain Python by tests/downsample_reference.py; mix64 is csrc/mix64.h and the draw is
 * csrc/downsample_draw.h.  All arithmetic is exact, unsigned 64-bit and modulo 2^64.
 *   G = 0x9e3779b97f4a7c15
 *   stream(seed, key)  = mix64(key ^ mix64(seed ^ G))                  seed: any uint64
 *   draw(seed, key, j) = mix64(stream(seed, key) + (j + 1) * G) >> 32  j = 0, 1, ...: the j-th read
 * Read j of a molecule is kept at threshold T (0 <= T <= 2^32) exactly when draw < T;
 * thin(seed, key, r, T) is the number of j < r that are kept.  T = 0 keeps nothing, T = 2^32
 * everything, and a fraction f is the threshold round(f * 2^32).  The draw depends on (seed, key, j)
 * only -- not on a slot, the capacity or the order of updates and merges -- so two counters with the
 * same contents thin to the same table, and for one seed what is kept at T1 <= T2 is a subset of what
 * is kept at T2: a curve is monotone by construction.
 * Reads that never became molecules are thinned by the same rule under keys no molecule can have: the
 * n reads of tally k (0 no match, 1 ambiguous, 2 bad UMI, 3 no feature) use key 2^63 | k, and
 * thin_tally(seed, k, n, T) is the number of j < n with draw(seed, 2^63 | k, j) < T.
 * downsample(dst, src, T, seed) is merge's sibling: afterwards dst is the counter that was fed dst's
 * updates followed by the thinned src.  For every key stored in src, m = thin(seed, key, mreads, T);
 * if m > 0 the key is claimed in dst by the update's own rule (molecules[index] += 1 from the lane
 * whose compare-and-swap took the slot, and from no other), mreads of the key in dst += m and
 * reads[index] += m; a molecule with m == 0 leaves no trace.  tally[k] += thin_tally(seed, k,
 * src.tally[k], T) for each of the four tallies, and total grows by the kept molecule reads plus the
 * kept tallies: reads of src that rule 3 refused (an index out of range) are in src.total only and
 * are not carried.  src is unchanged and stays usable; the same call twice adds the same reads again
 * and no molecule.  The result is an ordinary counter: collapse, the directional clusters, matrix,
 * merge and a further downsample work on it.
 * Conditions: dst != src; both counted; nw, kind, L and nf equal (merge's messages); T <= 2^32; both
 * on one device (for two, downsample on the source's device and then merge: the message says so).
 * A NULL counter or a violated condition is SCT_E_INVALID, a src whose table overflowed SCT_E_RANGE;
 * after any of these both counters are as they were.  Growth: the surviving molecules are counted
 * first (the curve pass below at the one threshold) and dst is grown by update's rehash so that
 * dst.nmolecules + survivors <= capacity / 2, merge's rule on the survivors and not on src's size: a
 * 10 % sample of a large table gets a small one.  More than 2^31 slots is SCT_E_RANGE.  The call
 * orders itself after both counters' earlier work on any stream and their later work after itself,
 * and waits for `stream` to learn the sizes and the kept reads (total is a host word).
 * downsample_curve: the whole curve in one pass over the table, nothing is built.  thresholds is a
 * host array of k integers, 1 <= k <= 64, none above 2^32 and none below the one before it (else
 * SCT_E_INVALID).  reads[t] = the sum of thin(seed, key, mreads, thresholds[t]) over the stored
 * molecules, molecules[t] = the stored molecules with thin > 0 there; both uint64[k], each nullable,
 * written and not accumulated; tallies are no part of the curve.  reads[t] and molecules[t] equal the
 * sums of reads[] and molecules[] after downsample(thresholds[t]) into an empty counter.  It needs a
 * counted counter (else SCT_E_INVALID), reads the table only (twice gives the same answer) and is
 * asynchronous on `stream` after one wait for the size; the _host form stages its outputs. */
int sct_molecules_downsample(sct_molecules* dst, sct_molecules* src, uint64_t threshold, uint64_t seed, void* stream);
int sct_molecules_downsample_curve(sct_molecules* mol, const uint64_t* thresholds, int64_t k, uint64_t seed,
                                   uint64_t* d_reads, uint64_t* d_molecules, void* stream);
int sct_molecules_downsample_curve_host(sct_molecules* mol, const uint64_t* thresholds, int64_t k, uint64_t seed,
                                        uint64_t* reads, uint64_t* molecules);

/* Removing swapped molecules: libraries multiplexed on one patterned-flowcell lane exchange a share of
 * their molecules by index hopping, and the same (cell barcode, UMI, feature) then shows up in two
 * samples.  The rule is DropletUtils' swappedDrops: the sample that holds at least num / den of a
 * molecule's reads over the samples of the lane keeps it, every other sample loses it, and when no
 * sample reaches the fraction all lose it.  This is the step between downsample (equal depth) and
 * merge (one table).  The contract is restated in plain Python by tests/swapped_reference.py; the
 * judgement is csrc/swapped_keep.h.  All arithmetic is exact; nothing is computed modulo 2^64.
 * The call takes s counters src[0 .. s), 1 <= s <= 16, all counted, with equal nw, kind, L and nf, on
 * one device, and judges the molecules of src[k].  For the molecule `key` stored in src[k] with
 * r = mreads:
 *   others = the sum of mreads of `key` in every src[t], t != k (0 where it is not stored), as a
 *            saturating add at 2^64 - 1;
 *   the molecule is *shared* when others > 0;
 *   it is *kept* exactly when r * (den - num) >= num * others, compared in the integers (both
 *   products are below 2^96: a high and a low word) -- r / (r + others) >= num / den with no
 *   division.  others == 0 always keeps; num == den keeps the unshared molecules only.
 * 1 <= num <= den <= 2^32 and 2 * num > den, so at most one sample keeps a key.  Keys are compared
 * whole: in a feature counter the feature is part of the molecule, as in swappedDrops, and the same
 * (index, UMI) under two features in two samples is not shared; without features the molecule is
 * (index, UMI).  No UMI collapse is applied before the judgement: a one-base variant of a swapped UMI
 * is its own key and is judged on its own reads.  The cleaned counter supports collapse afterwards.
 * Afterwards dst is the counter that was fed dst's updates followed by the kept molecules of src[k]
 * (downsample's wording and rule): every kept key is claimed in dst by the update's own rule
 * (molecules[index] += 1 from the lane whose compare-and-swap took the slot, and from no other),
 * mreads of the key in dst += r and reads[index] += r; a removed molecule leaves no trace.
 * dst.tally[j] += src[k].tally[j] for all four tallies -- those reads are not molecules and are not
 * judged -- and total grows by the kept reads plus the carried tallies; reads of src[k] that rule 3
 * refused are not carried, as in downsample.  tally (a host uint64[3], nullable) is written, not
 * accumulated: the shared molecules of src[k], the removed ones, and the reads of the removed ones.
 * No src is changed; the same call twice adds the same reads again and no molecule.
 * Growth: the survivors are known after the marking pass, before anything is claimed, and dst is
 * grown by update's rehash so that dst.nmolecules + survivors <= capacity / 2 -- merge's rule on the
 * survivors, not on the source's size; more than 2^31 slots is SCT_E_RANGE.
 * SCT_E_INVALID: a NULL pointer, s or k out of range, the same counter twice in src, dst among src, a
 * counter without read counts, differing parameters (merge's messages), two devices ("merge each into
 * a counter on one device first"), a bad num / den.  A src whose table overflowed is SCT_E_RANGE.
 * After any of these every counter is as it was.
 * The call orders itself after every involved counter's earlier work on any stream and their later
 * work after itself, and waits for `stream` once, to learn the survivors and the tally.  The other
 * samples' tables are probed in place, read-only; no union table is built. */
int sct_molecules_swapped(sct_molecules* const* src, int64_t s, int64_t k, sct_molecules* dst, uint64_t num,
                          uint64_t den, uint64_t* tally /* host uint64[3], nullable */, void* stream);

/* Counting molecules per feature: the barcode x feature matrix of a single-cell run -- molecules per
 * (cell, antibody tag / CRISPR guide / hashtag / gene) -- as CSR on the device.  The contract is
 * restated in plain Python by tests/count_matrix_reference.py.
 * A *feature counter* (sct_molecules_create_features) is a molecule counter made for nw barcodes and
 * nf features, 1 <= nf < 2^31 (else SCT_E_INVALID); flags and device are create_ex's, and create_ex
 * itself makes what it made before.  With feat_bits = max(1, bit_length(nf - 1)), the rule of
 * idx_bits, a key is (((index << feat_bits) | feature) << umi_bits) | umi, and
 * idx_bits + feat_bits + umi_bits <= 63 is required (else SCT_E_INVALID; the message names the three
 * widths), so the top bit stays 0 and EMPTY is never a key.  In practice: a 737K whitelist (20 bits)
 * with a ThreeBit 10-base UMI (30 bits) leaves 13 feature bits, enough for tag and guide panels;
 * gene-sized nf needs TwoBit UMIs -- 3.7M barcodes (22 bits) and 12 TwoBit bases (24 bits) leave 17.
 * update_features takes feature[i] (int32) beside index[i] and umi[i]: the feature's index as
 * sct_nearest_correct leaves it for a tag read, or a gene index from any aligner.  For read i, in
 * this order:
 *   1-3.  the rules of index, unchanged;
 *   3b.   feature outside [-2, nf):  not counted, nothing is stored through it, and the call is
 *                                    SCT_E_RANGE; the rest of the batch is counted;
 *   4.    a bad UMI, unchanged (tally[2]);
 *   4b.   feature == -1 or -2 (a tag that could not be placed): n_no_feature += 1, the fourth tally;
 *                                    the read counts nowhere else;
 *   5.    otherwise                  reads[index] += 1, and molecules[index] += 1 when the three-part key
 *                                    is new.
 * The same UMI under two features of one cell is two molecules (choosing one feature for such a
 * pair is not done here: see "resolving features" below).  Invariant: reads[nw] and molecules[nw] stay per barcode, and the row sums
 * of the matrix below equal them (and collapse's collapsed[nw] the row sums of the collapsed values).
 * The two-array sct_molecules_update(_host) on a feature counter is SCT_E_INVALID, and so is
 * update_features(_host) on a counter without features; both change nothing.  n == 0 changes nothing
 * and needs no pointer.  features_info: nf (0 for a counter without features) and n_no_feature, each
 * nullable; sct_molecules_counts* keeps writing 3 tally words.
 * Everything else holds for a feature counter unchanged: growth, streams, devices, info, counts,
 * counted-ness (mreads per three-part key), and
 *   fetch / fetch_counted   the same rows without the feature column, in ascending key order (so a
 *                           (index, umi) pair appears once per feature it was seen under);
 *   collapse                neighbours change UMI bits only, so a molecule's parent lies under its own
 *                           (index, feature); collapsed[index] is per barcode;
 *   merge                   nf must be equal too (the message names it).
 * fetch_features: fetch's rows with the feature column, ascending by barcode, then feature, then UMI
 * code; d_mreads and d_parent are nullable, and either one non-NULL needs a counted counter (else
 * SCT_E_INVALID).  The room rule is fetch's.
 * matrix: the state at the call, written and not accumulated, as CSR over nw rows:
 *   indptr     int64[nw + 1];
 *   feature    int32[nnz], ascending within a row;
 *   molecules  [nnz] the distinct UMIs of entry e;
 *   reads      [nnz] the sum of their mreads;
 *   collapsed  [nnz] the distinct parent values over the entry's molecules (a parent always lies in its
 *              child's entry, so the three value arrays share indptr and feature).
 * Each value array is nullable; reads or collapsed non-NULL on a counter that is not counted is
 * SCT_E_INVALID.  nnz (a host word, never NULL) is written whenever the call got as far as counting
 * the entries: room < nnz is SCT_E_INVALID with nnz reported, nothing else written and the counter
 * as it was.  nnz <= nmolecules, so room = nmolecules always suffices.  feature may be NULL only
 * when room == 0.  The call reads the table only: twice gives the same answer.  It waits for the
 * stream once (to learn nnz), as fetch does to learn nmolecules.  On a counter without features
 * fetch_features and matrix are SCT_E_INVALID. */
int sct_molecules_create_features(int64_t nw, int64_t nf, int kind, int L, int64_t capacity_hint, int flags,
                                  int device, sct_molecules** mol);
int sct_molecules_update_features(sct_molecules* mol, const int32_t* d_index, const int32_t* d_feature,
                                  const uint64_t* d_umi, int64_t n, void* stream);
int sct_molecules_update_features_host(sct_molecules* mol, const int32_t* index, const int32_t* feature,
                                       const uint64_t* umi, int64_t n);
int sct_molecules_features_info(sct_molecules* mol, int64_t* nf, int64_t* n_no_feature);
int sct_molecules_fetch_features(sct_molecules* mol, int32_t* d_index, int32_t* d_feature, uint64_t* d_umi,
                                 uint64_t* d_mreads, uint64_t* d_parent, int64_t room, void* stream);
int sct_molecules_fetch_features_host(sct_molecules* mol, int32_t* index, int32_t* feature, uint64_t* umi,
                                      uint64_t* mreads, uint64_t* parent, int64_t room);
int sct_molecules_matrix(sct_molecules* mol, int64_t* d_indptr, int32_t* d_feature, uint64_t* d_molecules,
                         uint64_t* d_reads, uint64_t* d_collapsed, int64_t room, int64_t* nnz, void* stream);
int sct_molecules_matrix_host(sct_molecules* mol, int64_t* indptr, int32_t* feature, uint64_t* molecules,
                              uint64_t* reads, uint64_t* collapsed, int64_t room, int64_t* nnz);
/* the same with a collapse method ("directional clusters" above) */
int sct_molecules_fetch_features_by(sct_molecules* mol, int method, int32_t* d_index, int32_t* d_feature,
                                    uint64_t* d_umi, uint64_t* d_mreads, uint64_t* d_parent, int64_t room,
                                    void* stream);
int sct_molecules_fetch_features_by_host(sct_molecules* mol, int method, int32_t* index, int32_t* feature,
                                         uint64_t* umi, uint64_t* mreads, uint64_t* parent, int64_t room);
int sct_molecules_matrix_by(sct_molecules* mol, int method, int64_t* d_indptr, int32_t* d_feature,
                            uint64_t* d_molecules, uint64_t* d_reads, uint64_t* d_collapsed, int64_t room,
                            int64_t* nnz, void* stream);
int sct_molecules_matrix_by_host(sct_molecules* mol, int method, int64_t* indptr, int32_t* feature,
                                 uint64_t* molecules, uint64_t* reads, uint64_t* collapsed, int64_t room,
                                 int64_t* nnz);

/* Resolving features: a (cell, UMI) pair is one physical molecule, and when it shows up under several
 * features -- a chimeric PCR product, an index hop, a mis-assigned read -- at most one of them keeps
 * it.  The rule is Cell Ranger's: after UMI correction, of the read groups that share barcode and
 * UMI the feature with the most reads keeps the molecule and the others are discarded; on a tie for
 * the most reads all of them are discarded.  The contract is restated in plain Python by
 * tests/feature_resolve_reference.py, and that restatement is the contract (the directional roots
 * follow this library's tie rule, the larger code, not UMI-tools' insertion order).
 * Input: a counted feature counter (SCT_MOLECULES_COUNTED, sct_molecules_create_features); anything
 * else is SCT_E_INVALID and changes nothing.
 * Method: SCT_COLLAPSE_ONE_STEP, SCT_COLLAPSE_DIRECTIONAL or SCT_COLLAPSE_NONE; any other value is
 * SCT_E_INVALID.  SCT_COLLAPSE_NONE is taken by the entry points of this block only: every *_by call
 * goes on rejecting it.
 * Image: every stored key (index, feature, umi) has an image under its own (index, feature): itself
 * (NONE), its one-step parent (ONE_STEP, "collapsing UMIs one base apart") or its directional root
 * (DIRECTIONAL, "directional clusters").
 * Collapsed molecule: (index, feature, image umi); its reads are the sum of mreads over the keys with
 * that image.  Collapse comes first: the groups are formed on the images and compared by the summed
 * reads.
 * Group: the collapsed molecules that share (index, image umi), over all features.  With top the
 * largest reads in the group: if exactly one member has top it is *kept* and the others are *lost*;
 * if two or more have top, every member of the group is *tied*, the members below top included, and
 * none is kept.  A group of one member keeps it.
 * Example: barcode 0, a UMI A and A' one base from it; feature 1 has A x 1 and A' x 3, feature 2 has
 * A' x 3.  NONE: A' ties 3 : 3 and both members drop, A stays: entry (0, 1) = 1, tally (1, 0, 2, 6).
 * ONE_STEP and DIRECTIONAL: feature 1's image A' carries 4 reads and beats feature 2's 3:
 * entry (0, 1) = 1, tally (1, 1, 0, 3).  Entry (0, 2) is an explicit 0 under every method.
 * Outputs, all written and not accumulated:
 *   resolved[nw]  (uint64) the kept molecules per barcode;
 *   tally[4]      (uint64, nullable) n_shared = the groups of at least 2 members, n_lost, n_tied, and
 *                 reads_dropped = the reads of the lost and tied members;
 *   matrix_resolved: sct_molecules_matrix_by's outputs and rules (room, nnz, the nullable value
 *                 arrays, the single wait for the stream) and resolved[nnz], the kept molecules of
 *                 entry (index, feature).  It shares indptr and feature with molecules, reads and
 *                 collapsed, so an entry that loses everything holds an explicit 0.  collapsed
 *                 non-NULL with SCT_COLLAPSE_NONE is SCT_E_INVALID.  room < nnz reports nnz and
 *                 writes nothing, the tally included.
 * An empty counter gives zeros and an indptr of zeros.  The calls read the table only: twice gives
 * the same answer, and molecules, collapsed, counts and every other call mean what they meant.
 * Invariants:
 *   sum(resolved) + n_lost + n_tied == sum(collapsed) of the same method (nmolecules for NONE);
 *   the row sums of the matrix's resolved[nnz] are resolved[nw];
 *   resolved[e] <= collapsed[e] for every entry (<= molecules[e] for NONE);
 *   with n_shared == 0, resolved equals collapsed entry for entry and the other tally words are 0;
 *   the answer depends on the table's contents (key -> reads) only: not on the order of updates, the
 *   capacity, the growth history, or whether the table came from merge or downsample.
 * Every value is an exact integer.  The device forms order themselves after the counter's earlier
 * work, as every call does; DIRECTIONAL waits for the stream between its sweeps.  Scratch, from the
 * library's pool in one block: the sorted rows (24 B per molecule and the sort's own), 1 bit per slot,
 * 4 B per slot for ONE_STEP (the images) or the directional pass's scratch for DIRECTIONAL. */
#define SCT_COLLAPSE_NONE 2
int sct_molecules_resolve(sct_molecules* mol, int method, uint64_t* d_resolved, uint64_t* d_tally, void* stream);
int sct_molecules_resolve_host(sct_molecules* mol, int method, uint64_t* resolved, uint64_t* tally);
int sct_molecules_matrix_resolved(sct_molecules* mol, int method, int64_t* d_indptr, int32_t* d_feature,
                                  uint64_t* d_molecules, uint64_t* d_reads, uint64_t* d_collapsed,
                                  uint64_t* d_resolved, uint64_t* d_tally, int64_t room, int64_t* nnz,
                                  void* stream);
int sct_molecules_matrix_resolved_host(sct_molecules* mol, int method, int64_t* indptr, int32_t* feature,
                                       uint64_t* molecules, uint64_t* reads, uint64_t* collapsed,
                                       uint64_t* resolved, uint64_t* tally, int64_t room, int64_t* nnz);

/* Read groups: every read tagged with its molecule.  The calls above answer per barcode or per matrix
 * entry; a read-groups object answers per read -- the corrected UMI of the read (the UB tag, the output
 * of `umi_tools group`), whether its molecule survived "resolving features", how many reads the
 * molecule has and whether the read is the first of it (duplicate marking).  The contract is restated
 * in plain Python by tests/read_groups_reference.py, and that restatement is the contract.
 * Create: a *snapshot* of the counter `mol` as it stands on `stream`, under `method`
 * (SCT_COLLAPSE_NONE, SCT_COLLAPSE_ONE_STEP or SCT_COLLAPSE_DIRECTIONAL; the images are those of
 * "resolving features") and `flags`:
 *   SCT_GROUPS_RESOLVED  the final molecules that sct_molecules_resolve(method) does not keep give
 *                        SCT_READ_LOST; needs a counted feature counter;
 *   SCT_GROUPS_READS     tag writes the reads of every read's final molecule; needs a counted counter;
 *   SCT_GROUPS_FIRST     tag marks the first read of every final molecule.
 * A collapsing method needs a counted counter.  Anything else is SCT_E_INVALID.  The object owns
 * every array tag reads: the counter may afterwards be updated, grown, merged into or destroyed, and
 * tag goes on giving the snapshot's answers.  It lives on the counter's device; every call works
 * whatever device is current and leaves it as it was.  Create waits for `stream` (it reads the size;
 * DIRECTIONAL also between its sweeps).
 * Final molecule of a stored key (index, feature, umi): (index, feature, image umi).  Its reads: the
 * sum of mreads over the stored keys with that image -- one step, not followed further.
 * Tag: per read, in this order of precedence,
 *   index == -1                                        SCT_READ_NO_BARCODE
 *   index == -2                                        SCT_READ_AMBIGUOUS
 *   index outside [-2, nw) or feature outside [-2, nf) SCT_READ_BAD_INDEX
 *   a bad UMI (as sct_molecules_update's rule)         SCT_READ_BAD_UMI
 *   feature < 0                                        SCT_READ_NO_FEATURE
 *   the key is not stored in the snapshot              SCT_READ_ABSENT (a UMI one base from a stored
 *                                                      one is not corrected: only stored keys have images)
 *   RESOLVED and the final molecule is not kept        SCT_READ_LOST
 *   otherwise                                          SCT_READ_GROUPED
 * final_umi is the image UMI for LOST and GROUPED and the input UMI otherwise; reads is the final
 * molecule's reads for LOST and GROUPED and 0 otherwise.  d_feature is NULL exactly when the counter has
 * no features; d_reads / d_first are non-NULL exactly when the flag asked for the column (SCT_E_INVALID
 * otherwise).
 * First: every read given to tag gets an ordinal, the number of reads the object was given before it
 * (of any status; position in a call and the order of the calls both count).  first is 1 for exactly
 * one read of every final molecule that has a GROUPED read, the one with the lowest ordinal, and 0 for
 * every other read.  It depends on neither the table layout, the launch shape nor the batch cut.
 * A batch with a BAD_INDEX read is tagged whole, the ordinals advance by the whole batch, and then the
 * call returns SCT_E_RANGE.  tag waits for `stream` once (it reads the tallies back to learn that).
 * Calls on different streams are ordered by an event, as a counter's are.  An empty counter gives
 * SCT_READ_ABSENT for every otherwise good read.
 * info: the reads given to tag so far, and tally[8] (nullable), the reads per status.
 * Invariants, when every counted read is tagged exactly once: count(first) is sum(molecules),
 * sum(collapsed) of the method, or sum(resolved) with RESOLVED; count(LOST) == reads_dropped; and the
 * reads of the first reads' molecules + reads_dropped == sum(reads).
 * Memory: 16 B per table slot (the keys, and a word with the final UMI and the kept flag), 8 B more for
 * READS and 12 B more for FIRST (the lowest ordinal, and the image's slot). */
#define SCT_GROUPS_RESOLVED 1
#define SCT_GROUPS_READS 2
#define SCT_GROUPS_FIRST 4
#define SCT_READ_GROUPED 0
#define SCT_READ_NO_BARCODE 1
#define SCT_READ_AMBIGUOUS 2
#define SCT_READ_BAD_UMI 3
#define SCT_READ_NO_FEATURE 4
#define SCT_READ_ABSENT 5
#define SCT_READ_LOST 6
#define SCT_READ_BAD_INDEX 7
typedef struct sct_read_groups sct_read_groups;
int sct_read_groups_create(sct_molecules* mol, int method, int flags, sct_read_groups** groups, void* stream);
int sct_read_groups_tag(sct_read_groups* g, const int32_t* d_index, const int32_t* d_feature, const uint64_t* d_umi,
                        int64_t n, uint64_t* d_final_umi, uint8_t* d_status, uint64_t* d_reads, uint8_t* d_first,
                        void* stream);
int sct_read_groups_tag_host(sct_read_groups* g, const int32_t* index, const int32_t* feature, const uint64_t* umi,
                             int64_t n, uint64_t* final_umi, uint8_t* status, uint64_t* reads, uint8_t* first);
int sct_read_groups_info(sct_read_groups* g, int64_t* tagged, uint64_t* tally);
int sct_read_groups_destroy(sct_read_groups* g);

/* ---------------------------------------------------------------- FASTQ barcode extraction
 * Replaces the per-record path reader.Reader.__iter__ (src/sctools/reader.py:56-85) ->
 * fastq.Reader.record_grouper (src/sctools/fastq.py:143-150) -> Record name check
 * (fastq.py:31-38) -> EmbeddedBarcodeGenerator / extract_barcode (fastq.py:181-200):
 * record.sequence[start:end] and record.quality[start:end] of every record.
 * The input is the files' bytes concatenated (file_ends = cumulative end offsets, the last
 * == nbytes; a record may span files, an incomplete trailing record is dropped).  Lines
 * keep their newline, so slices of short reads include '\n' exactly as in Python.
 * text_mode = 0 is open(..., 'rb'): lines end at '\n'; 1 is 'r': '\n', "\r\n" and a lone
 * '\r' each end a line and read back as '\n' (ASCII input only, else SCT_E_RANGE).
 * first_bad_name = the first record whose name line does not start with '@' (the
 * reference raises ValueError('fastq name must start with @') there), or -1.
 */
typedef struct sct_fastq_index sct_fastq_index;
/* The count stage, synchronous: every 8 KiB tile's line count and first line end, and the counts
 * summed over blocks of 32 and 1,024 tiles (-> nrecords = lines / 4); nothing per line is kept.
 * The buffer must stay alive and unchanged until the index is destroyed.  One launch covers the
 * buffer, as in sct_fastq_extract_fused: tiles * 256 < 2^32, about 137 GB (SCT_E_INVALID, "buffer
 * too large", beyond it; the stream form passes a file in pieces). */
int sct_fastq_index_create(const uint8_t* d_buf, int64_t nbytes, const int64_t* file_ends, int nfiles,
                           int text_mode, void* stream, sct_fastq_index** index);
int sct_fastq_index_destroy(sct_fastq_index* index);
/* first_bad_name: from the last sct_fastq_extract_spans (-2 before any). */
int sct_fastq_index_info(const sct_fastq_index* index, int64_t* nrecords, int64_t* nlines,
                         int64_t* first_bad_name);
/* The range stage on an index, synchronous: every record's sequence-line and quality-line
 * slices for all spans (nspans <= 8 host (start, end) pairs, end <= 4096) and the '@' check of
 * every name line.
 * Span k's rows start at d_seq / d_qual + nrecords * sum_{i<k} width_i (zero padded rows of
 * width_k), lengths at d_seq_len / d_qual_len + k * nrecords; every output is nullable. */
int sct_fastq_extract_spans(sct_fastq_index* index, const uint8_t* d_buf, const int32_t* spans,
                            int nspans, uint8_t* d_seq, uint8_t* d_qual, int32_t* d_seq_len,
                            int32_t* d_qual_len, int64_t* first_bad_name, void* stream);
/* Index and extraction in one call (the same count and range stages; asynchronous on
 * `stream`, no host synchronisation): d_file_ends is DEVICE memory; rows are laid out by the
 * caller's capacity (span k's row r at out + cap_records * prefix_k + r * width_k; lengths at
 * len + k * cap + r; records >= cap_records are not written); d_status (3 int64, device): [0]
 * line count (records = lines / 4), [1] ~(first bad-name record) or 0, [2] non-ASCII seen (text
 * mode rejects it).  d_codes0 / d_gc0 / d_flags0 (nullable): span 0's sequence rows encoded as
 * sct_encode(code_kind) would encode those rows (code_kind 2 TwoBit, width <= 32; 3 ThreeBit,
 * width <= 21 -- N kept, the queries of sct_nearest_query). */
int sct_fastq_extract_fused(const uint8_t* d_buf, int64_t nbytes, const int64_t* d_file_ends, int nfiles,
                            int text_mode, const int32_t* spans, int nspans, int64_t cap_records, uint8_t* d_seq,
                            uint8_t* d_qual, int32_t* d_seq_len, int32_t* d_qual_len, uint64_t* d_codes0,
                            uint8_t* d_gc0, uint8_t* d_flags0, int code_kind, int64_t* d_status, void* stream);
/* Host convenience: spans = nspans (start, end) pairs.  Call with max_records < the record
 * count to learn nrecords (outputs untouched); then with room for nrecords:
 * seq_out/qual_out (nullable) = span k's rows at offset sum_{i<k} nrecords*width_i,
 * seq_len/qual_len (nullable) = nspans x nrecords lengths. */
int sct_fastq_extract_host(const uint8_t* buf, int64_t nbytes, const int64_t* file_ends, int nfiles,
                           int text_mode, const int32_t* spans, int nspans, uint8_t* seq_out,
                           uint8_t* qual_out, int32_t* seq_len, int32_t* qual_len,
                           int64_t max_records, int64_t* nrecords, int64_t* first_bad_name);

/* Streaming form (reader.Reader reads its files lazily, reader.py:56-85): a stream keeps
 * its device buffers across pieces of the concatenated files.  Each piece must end on a
 * '\n' unless final; file_ends are the files' ends inside the piece (the last == nbytes).
 * chunk: extracts every complete record of the piece on the device; consumed = the byte
 * just past the last complete record (final = 1: nbytes, the incomplete tail dropped);
 * the caller starts the next piece there.  fetch: that piece's outputs, laid out as
 * sct_fastq_extract_host's (each nullable; qualities only if the stream keeps them). */
typedef struct sct_fastq_stream sct_fastq_stream;
int sct_fastq_stream_create(int text_mode, const int32_t* spans, int nspans, int qualities,
                            sct_fastq_stream** stream);
int sct_fastq_stream_destroy(sct_fastq_stream* stream);
int sct_fastq_stream_chunk(sct_fastq_stream* stream, const uint8_t* buf, int64_t nbytes, const int64_t* file_ends,
                           int nfiles, int final, int64_t* nrecords, int64_t* consumed, int64_t* first_bad_name);
int sct_fastq_stream_fetch(sct_fastq_stream* stream, uint8_t* seq_out, uint8_t* qual_out, int32_t* seq_len,
                           int32_t* qual_len);
/* Copy the NEXT piece to the device ahead of its chunk call (asynchronous, on a copy stream of
 * the stream's own): a caller that knows the next piece while it works on this one's results
 * overlaps the piece's PCIe copy with that work.  Only a page-locked piece (sct_host_pinned) is
 * staged (anything else: a no-op); the piece's bytes must stay unchanged until the chunk call
 * for exactly (buf, nbytes) -- which then skips its own copy -- or the next stage call, or
 * the stream's destruction (each waits for the copy). */
int sct_fastq_stream_stage(sct_fastq_stream* stream, const uint8_t* buf, int64_t nbytes);

/* ---------------------------------------------------------------- bench aid
 * Streaming device copy (16 B per lane, nontemporal, resident grid) of `bytes` (a multiple
 * of 16): the practical HBM ceiling bench.py prices the kernels against beside the spec. */
int sct_stream_copy(void* d_dst, const void* d_src, int64_t bytes, void* stream);

/* ---------------------------------------------------------------- summary
 * Replaces barcode.py:44-46 (np.percentile(distances,[0,25,50,75,100]) with numpy's
 * default 'linear' method, then np.mean) computed from the histogram alone,
 * bit-exact in float64.  out[0..5] = minimum, 25th percentile, median,
 * 75th percentile, maximum, average.  Returns SCT_E_RANGE when the histogram is
 * empty (the reference raises IndexError).
 */
int sct_summary_from_hist(const uint64_t* hist, int nbins, double* out);

#ifdef __cplusplus
}
#endif

#endif /* SCTOOLS_HIP_H */
