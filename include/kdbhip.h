/*
 * kdbhip.h -- C ABI of libkdbhip.so, the MI355X (gfx950) k-mer counting engine
 * that replaces the inner loops of kmerdb's `profile` hot path.
 *
 * The reference (MatthewRalston/kmerdb v0.9.6) is pure Python and has no FFI:
 * its boundary for this path is the Python function
 *     kmerdb/parse.py:90   parsefile(filepath, k, replace_with_none, canonicalize)
 * whose body (parse.py:117-137) loops  kmer.shred -> kmer.kmer_to_id  per
 * window and does  counts[kmer_id] += 1.  Every entry point below cites the
 * reference lines whose work it takes over.  Plain pointers and sizes only;
 * no torch / numpy types.  The ctypes stub a kmerdb maintainer would add is
 * shown in INTEGRATION.md; kmerdb_amd/_abi.py is that stub.
 *
 * Threading: one producer thread per engine handle.  All functions return an
 * int status (KDB_OK == 0); kdb_last_error() gives a thread-local message.
 */
#ifndef KDBHIP_H
#define KDBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDB_ABI_VERSION 6

/* status codes */
#define KDB_OK               0
#define KDB_ERR_ARG          1   /* bad argument (reference: TypeError / ValueError at parse.py:109-116) */
#define KDB_ERR_HIP          2   /* a HIP runtime call failed; message has hipGetErrorString */
#define KDB_ERR_SHORT_READ   3   /* a record shorter than k   (reference raises: kmer.py:461-463) */
#define KDB_ERR_BAD_RESIDUE  4   /* a byte outside "ACGTN"    (reference raises: kmer.py:309 KeyError, :170 NameError) */
#define KDB_ERR_NOMEM        5   /* 4^k table or staging does not fit on the device */
#define KDB_ERR_STATE        6   /* call sequence error */

/* N handling == the reference's `replace_with_none` flag (kmer.py:541-565) */
#define KDB_N_DROP    0          /* replace_with_none=True : windows containing N emit nothing          */
#define KDB_N_EXPAND  1          /* replace_with_none=False: a window with m N's emits all 4^m fills    */

typedef struct kdb_engine kdb_engine;

int         kdb_abi_version(void);
const char *kdb_last_error(void);
int         kdb_device_count(int *n_out);

/*
 * Create an engine on `device_id` holding a dense 4^k uint64 count vector in
 * HBM, zeroed.  Replaces  counts = np.zeros(4**k, dtype="uint64")  parse.py:117-120.
 * `d_table` may be NULL (engine hipMallocs and owns the vector) or a device
 * pointer to 4^k uint64 owned by the caller (e.g. a torch tensor that will be
 * handed to RCCL afterwards); it is zeroed by kdb_create either way.
 * A caller's d_table must be 16-byte aligned (KDB_ERR_ARG otherwise): the histogram pass of the paged paths adds to the
 * vector in 16-byte pieces, and which path counts a batch is only decided when the batch arrives.  The engine reads and
 * writes the 4^k entries and nothing beside them.
 * 1 <= k <= 17 (4^17 * 8 B = 128 GiB; larger tables do not fit 288 GB).
 */
int kdb_create(int k, int canonicalize, int n_mode, int device_id, void *d_table, kdb_engine **out);
int kdb_destroy(kdb_engine *e);

/* Zero the count vector and the running totals (a new parsefile call). */
int kdb_reset(kdb_engine *e);

/*
 * Count every k-mer of `nreads` records.  Replaces the loop parse.py:128-137
 * (shred kmer.py:489-577 + kmer_to_id kmer.py:234-317 + counts[id] += 1).
 *   bases        : raw ASCII residues of all records, concatenated (no separators)
 *   read_offsets : nreads+1 offsets; record r = bases[read_offsets[r] .. read_offsets[r+1])
 * Windows never span records.  Asynchronous: the call returns once the data is
 * staged into pinned memory; copies and kernels run on the engine's streams,
 * double-buffered.  The caller's buffers may be reused as soon as it returns.
 * Records longer than a staging buffer are tiled with a k-1 base overlap.
 */
int kdb_submit(kdb_engine *e, const uint8_t *bases, size_t nbytes,
               const uint64_t *read_offsets, size_t nreads);

/*
 * Same as kdb_submit for buffers in pinned host memory (kdb_host_alloc / hipHostMalloc): the DMA reads
 * `bases` directly, with no staging copy, so `bases` must stay valid and unmodified until kdb_sync /
 * kdb_finish returns -- or until two further kdb_submit_pinned calls have returned (call N first waits for the
 * copies of call N-2, so cycling through three buffers is safe).  `read_offsets` may be reused at once.
 */
int kdb_submit_pinned(kdb_engine *e, const uint8_t *bases, size_t nbytes,
                      const uint64_t *read_offsets, size_t nreads);
/*
 * kdb_submit / kdb_submit_pinned with flags.  KDB_SUBMIT_CONTINUES: record 0 of this call is the next piece of the
 * LAST record of the previous call (a FASTA record longer than the reader's block, kmerdb/parse.py:50-85 streams
 * whole genomes): the caller starts the piece with the last k-1 residues it submitted, so that every window is seen
 * once; the piece gets no record start and is not subject to the "shorter than k" check.
 */
#define KDB_SUBMIT_PINNED     1
#define KDB_SUBMIT_CONTINUES  2
int kdb_submit_ex(kdb_engine *e, const uint8_t *bases, size_t nbytes,
                  const uint64_t *read_offsets, size_t nreads, int flags);
int kdb_host_alloc(void **out, size_t nbytes);     /* pinned host memory for kdb_submit_pinned */
int kdb_host_free(void *p);

/*
 * Same, for inputs already resident in HBM on the engine's device (device
 * pointers; d_bases 16-byte aligned).  The LDS-histogram paths (the default) only
 * read both buffers: a ragged batch's record starts are taken from the offsets.
 * The direct-atomics kernel ("algo" 1, and the fallback when the scatter
 * scratch does not fit in HBM) sets bit 7 of the first byte of every record of
 * a ragged batch in d_bases (its in-HBM record-boundary mark; the low 7 bits
 * are untouched) while it reads the batch and clears it again afterwards, so the
 * buffer is unchanged once the stream has drained and may be submitted again
 * with other offsets.  The buffers must stay alive until kdb_sync / kdb_finish
 * returns.
 */
int kdb_submit_device(kdb_engine *e, void *d_bases, size_t nbytes,
                      const void *d_read_offsets, size_t nreads);

/*
 * kdb_submit_device for a buffer the engine must not write (shared read-only between engines or streams).  On the
 * LDS-histogram paths that is every batch.  Where the direct-atomics kernel has to run ("algo" 1, or no room for the
 * scatter scratch) a batch of ragged records makes kdb_sync / kdb_finish return KDB_ERR_ARG: that kernel marks record
 * starts in the buffer (records of one length need no marks: the usual FASTQ shape).
 */
int kdb_submit_device_const(kdb_engine *e, const void *d_bases, size_t nbytes,
                            const void *d_read_offsets, size_t nreads);

/* Wait for all submitted work; surfaces KDB_ERR_SHORT_READ / KDB_ERR_BAD_RESIDUE. */
int kdb_sync(kdb_engine *e);

/*
 * Sync, then copy the count vector to `counts_out` (4^k uint64, caller-owned,
 * may be NULL to skip the copy) and report the totals parsefile derives at
 * parse.py:139-147:  total_kmers (Sum counts), unique_kmers (count_nonzero).
 * Does not reset the engine: further submits keep accumulating (the
 * `counts = counts + counts_` of kmerdb/__init__.py:1890 stays on the device).
 */
int kdb_finish(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers);

/*
 * Like kdb_finish for a vector the engine did not fill alone -- after the RCCL reduce of SURVEY 8(e) rank 0's
 * vector holds every rank's counts, so Sum(counts) no longer equals what this engine emitted and kdb_finish's
 * internal consistency check does not apply.  Reports Sum(counts) and count_nonzero(counts) of the vector as it is.
 */
int kdb_table_stats(kdb_engine *e, uint64_t *counts_out, uint64_t *sum_out, uint64_t *unique_out);

/*
 * nullomer_array of parse.py:139-140 -- the ids whose count is zero, ascending -- by stream compaction on the device
 * (np.flatnonzero over the 2^30 bins of k = 15 costs the host 1.5 s; the device sweeps the vector twice at HBM speed and
 * sends back only the ids).  Syncs first.  `folded` = 0: the count vector, 1: the samplesheet accumulator (kdb_fold_file).
 * *n_out = number of such ids (4^k - count_nonzero); ids_out may be NULL to ask for the number alone, otherwise it holds
 * `cap` entries (KDB_ERR_ARG if fewer than *n_out, with *n_out set).
 */
int kdb_nullomers(kdb_engine *e, int folded, uint64_t *ids_out, uint64_t cap, uint64_t *n_out);

/*
 * The reduce of SURVEY 8(e) for ONE process that drives several GPUs (an engine per device, records dealt out
 * between them -- a record is counted independently of every other, parse.py:128-137): sum the count vectors of
 * engines[0..n) into engines[root]'s.  All engines are synced first (a KDB_ERR_SHORT_READ / KDB_ERR_BAD_RESIDUE
 * of any of them is returned and nothing is reduced).  The 4^k index range is cut into n slices: engine j sums
 * slice j of every vector over xGMI peer access (all links busy in both directions), then the root collects the
 * n - 1 finished slices -- 2 x (n-1)/n x 4^k x 8 bytes over the root's links instead of (n-1) x 4^k x 8.
 * Integer sums: the result is the single-GPU vector bit for bit.  Afterwards engines[root] also carries the k-mers
 * emitted by all of them, so kdb_finish(engines[root], ...) reports the job's totals; the other engines' vectors
 * are partly overwritten -- kdb_reset them before further use.  Same k for all, 2 <= n <= KDB_REDUCE_MAX, engines
 * distinct; engines on the same device are allowed (tests on a one-GPU box).  KDB_ERR_HIP if two of the devices
 * cannot reach each other's memory.  (One process per GPU -- torch.distributed / RCCL -- is the other form:
 * kmerdb_amd/distributed.py reduces the same vectors with dist.reduce in 1 GiB pieces, see INTEGRATION.md.)
 */
#define KDB_REDUCE_MAX 16
int kdb_reduce(kdb_engine *const *engines, int n, int root);

/*
 * The two strands of a profile, merged (csrc/kdb_strands.hip.h).  d_fwd holds 4^k forward counts, d_table 4^k counts; rc(i) reverses the k
 * two-bit digits of i and complements each.
 *   d_table[i] += d_fwd[i] + d_fwd[rc(i)]   for i <  rc(i)
 *   d_table[i] += d_fwd[i]                  for i == rc(i)
 *   d_fwd is all zero afterwards; bins of d_table with i > rc(i) are not touched.
 * A canonical engine does this itself at every kdb_sync (option "strand_merge"); the entry point runs the same kernels on any two
 * vectors of the caller's.  Both on device_id, 8-byte aligned, not the same vector; k = 1..17.  Returns after the kernel has finished.
 */
int kdb_strand_merge(int device_id, void *d_fwd, void *d_table, int k);

/*
 * Exact integer moments of n finished count vectors on one device, in one sweep (csrc/kdb_gram.hip.h): what every distance of
 * `kmerdb distance` on count profiles is a function of (kmerdb/__init__.py:577-813, distance.pyx:108-152; kmerdb_amd/distance.py).
 *   S[i]    = Sum_b x_i[b]            -> sums_out[2 i], [2 i + 1] = low, high 64 bits
 *   G[i][j] = Sum_b x_i[b] x_j[b]     -> gram_out[2 (i n + j)], [.. + 1]; both triangles are filled
 * d_vectors: n device pointers (a host array of them) to nbins uint64 each, 16-byte aligned, read only; the same pointer may appear
 * twice.  Synchronous; the caller has synchronised whatever produced the vectors; scratch is allocated and freed inside the call.
 * If every S[i] < 2^64 then G[i][j] <= S[i] S[j] < 2^128: 128-bit accumulation cannot wrap.  KDB_ERR_ARG: n < 1, n > KDB_GRAM_MAX,
 * nbins == 0 (or above 2^36: no device holds such a vector), a NULL or misaligned pointer, or some S[i] >= 2^64 (the sums are exact always; the products may have wrapped).
 * KDB_ERR_NOMEM: the scratch does not fit.  kernel_ms_out (may be NULL): device time of the sweep, by HIP events.
 * KDB_GRAM_BLOCK / KDB_GRAM_WG_BINS: the kernel's constants -- vectors per register block, bins one workgroup covers per grid stride.
 * KDB_GRAM_GRID_MAX / _MAX_MANY_ROWS / _MANY_ROWS: the most workgroups per row (a row: one pair of blocks here, a block against up to
 * KDB_PAIRSTATS_HALF vectors in kdb_pairstats, which shares the three) that sweep the whole chunks -- the first cap for a call of fewer
 * than KDB_GRAM_GRID_MANY_ROWS rows, the second from that many rows on.  A workgroup past its first KDB_GRAM_WG_BINS bins strides on by
 * grid x KDB_GRAM_WG_BINS.  Any grid gives the same integers; the tests take their shapes from these.
 */
#define KDB_GRAM_MAX 64
#define KDB_GRAM_BLOCK 4
#define KDB_GRAM_WG_BINS 512
#define KDB_GRAM_GRID_MAX 1024
#define KDB_GRAM_GRID_MAX_MANY_ROWS 256
#define KDB_GRAM_GRID_MANY_ROWS 4
int kdb_gram(int device_id, const void *const *d_vectors, int n, uint64_t nbins,
             uint64_t *sums_out   /* 2*n   words: lo, hi of S[i]            */,
             uint64_t *gram_out   /* 2*n*n words: lo, hi of G[i][j], both triangles filled */,
             double   *kernel_ms_out /* may be NULL: device time by HIP events */);

/*
 * What the distances that are not functions of the moments need, as exact integers, in one pairwise sweep of the same n vectors
 * (csrc/kdb_pairstats.hip.h): cityblock, chebyshev, braycurtis, hamming and the presence/absence family (kmerdb_amd/distance.py).
 *   S[i]   = Sum_b x_i[b]                    -> sums_out[2 i], [2 i + 1] = low, high 64 bits
 *   nnz[i] = #{b : x_i[b] > 0}               -> nnz_out[i]
 *   for every pair, at [i n + j] and [j n + i] alike (both triangles are filled):
 *   L1     = Sum_b |x_i[b] - x_j[b]|         -> l1_out[2 (i n + j)], [.. + 1] = low, high 64 bits
 *   Linf   = max_b |x_i[b] - x_j[b]|         -> linf_out[i n + j]
 *   ne     = #{b : x_i[b] != x_j[b]}         -> ne_out[i n + j]
 *   both   = #{b : x_i[b] > 0 and x_j[b] > 0} -> both_out[i n + j]
 *   on the diagonal L1 = Linf = ne = 0 and both = nnz[i].
 * d_vectors, the call's conventions and its refusals are those of the moments above: n device pointers to nbins uint64 each, 16-byte
 * aligned, read only, the same pointer may appear twice; synchronous; scratch allocated and freed inside the call.
 * L1 <= S[i] + S[j] < 2^65 once every S is below 2^64: it may pass one word, so it has two.  KDB_ERR_ARG: n < 1, n > KDB_GRAM_MAX,
 * nbins == 0 or above 2^36, a NULL or misaligned pointer, a NULL output, or some S[i] >= 2^64.  KDB_ERR_NOMEM: the scratch does not fit.
 * kernel_ms_out (may be NULL): device time of the sweep, by HIP events.
 * KDB_PAIRSTATS_BLOCK / _HALF / _WG_BINS: the kernel's constants -- vectors per register block, vectors of the second block a row takes
 * off the diagonal, bins one workgroup covers per grid stride.  The grid's caps are kdb_gram's (KDB_GRAM_GRID_*), by this call's rows.
 */
#define KDB_PAIRSTATS_BLOCK 4
#define KDB_PAIRSTATS_HALF 2
#define KDB_PAIRSTATS_WG_BINS 512
int kdb_pairstats(int device_id, const void *const *d_vectors, int n, uint64_t nbins,
                  uint64_t *sums_out  /* 2*n   words */, uint64_t *nnz_out  /* n   words */,
                  uint64_t *l1_out    /* 2*n*n words */, uint64_t *linf_out /* n*n words */,
                  uint64_t *ne_out    /* n*n   words */, uint64_t *both_out /* n*n words */,
                  double   *kernel_ms_out /* may be NULL */);

/*
 * The two pairwise sums that need a quotient or a logarithm per bin, in float64 (csrc/kdb_pairstats.hip.h), for every pair i != j:
 *   C = Sum_b |x - y| / (x + y) over the bins with x + y > 0                        -> canberra_out[i n + j]    (scipy's canberra)
 *   D = Sum_b [ p ln(p/m) + q ln(q/m) ], p = x/S[i], q = y/S[j], m = (p + q)/2      -> js_out[i n + j]          (scipy's jensenshannon is sqrt(D/2))
 * a zero p or q contributes 0; D is nan where S[i] or S[j] is 0; the diagonal of both is 0; both triangles are filled.
 * |x - y| is formed in integers; S are the exact sums (one integer sweep inside the call), converted to float64 once.  Each per-bin
 * term is non-negative and is formed before it is added; no atomics; the grid depends on nbins alone and the order of the additions is
 * fixed: two calls on the same vectors return the same bits (on one build; not promised across builds).  IEEE division: the library is
 * built without fast-math.  Conventions and refusals as above.  kernel_ms_out (may be NULL): device time of the float sweep alone.
 * KDB_PAIRFLOAT_GRID_MAX: the most workgroups per pair that sweep the whole chunks (KDB_PAIRSTATS_WG_BINS bins each per grid stride).
 */
#define KDB_PAIRFLOAT_GRID_MAX 512
int kdb_pairfloat(int device_id, const void *const *d_vectors, int n, uint64_t nbins,
                  double *canberra_out /* n*n */, double *js_out /* n*n */,
                  double *kernel_ms_out /* may be NULL */);

/*
 * Median-of-ratios size factors of the same n vectors (Anders & Huber 2010; DESeq2's estimateSizeFactors), csrc/kdb_sizefactors.hip.h:
 *   a bin b is eligible iff x_j[b] > 0 for every j;     L[b] = (1/n) Sum_j ln x_j[b] on eligible bins (j in order, float64)
 *   log_sf_out[j] = median over the eligible bins of ln x_j[b] - L[b]: the middle element, or the arithmetic mean of the two middle
 *   elements of an even number (R's and numpy's median);     *eligible_out = the number of eligible bins, exact.
 * The size factor is exp(log_sf_out[j]), left to the caller.  With no eligible bin the call returns KDB_OK, *eligible_out = 0 and nan in
 * log_sf_out.  The median is found by a radix select over keys recomputed from the vectors in every pass, never stored; all accumulation
 * across the device is integer, so two calls on the same vectors return the same bits, whatever the grid.  KDB_ERR_STATE if the passes
 * disagree (a vector changed during the call).  d_vectors, conventions and refusals as for the moments above; KDB_ERR_ARG also for a NULL
 * log_sf_out or eligible_out; KDB_ERR_NOMEM if the float64 scratch of nbins entries does not fit.  kernel_ms_out (may be NULL): device
 * time of the sweep and the select passes.
 * KDB_SIZEFACTORS_WG_BINS: bins one workgroup of these kernels covers per grid stride.  KDB_SIZEFACTORS_GRID_MAX: the most workgroups
 * (per sample) of a sweep, of kdb_scale_counts' too.
 */
#define KDB_SIZEFACTORS_WG_BINS 512
#define KDB_SIZEFACTORS_GRID_MAX 1024
int kdb_size_factors(int device_id, const void *const *d_vectors, int n, uint64_t nbins,
                     double *log_sf_out /* n */, uint64_t *eligible_out, double *kernel_ms_out /* may be NULL */);

/*
 * One vector divided by its size factor: d_out[b] = x[b] / size_factor in IEEE float64 (x converted round-to-nearest-even), rounded half
 * to even to an integer and stored as uint64 (as_float64 == 0: numpy's rint), or stored unrounded as float64 (as_float64 != 0).
 * d_out: nbins 8-byte entries on the same device, 16-byte aligned; it may be d_vector itself.  KDB_ERR_ARG: a NULL or misaligned pointer,
 * nbins == 0 or above 2^36, a size_factor that is not finite and > 0, or (integer output) a rounded quotient of 2^63 or more -- d_out is
 * then left as it was.  kernel_ms_out (may be NULL): device time.
 */
int kdb_scale_counts(int device_id, const void *d_vector, uint64_t nbins, double size_factor,
                     void *d_out /* may equal d_vector */, int as_float64, double *kernel_ms_out /* may be NULL */);

/*
 * The abundance spectrum of one finished count vector -- how many bins hold each count value -- in one sweep on the device
 * (csrc/kdb_spectrum.hip.h): the reference's util.get_histo (kmerdb/util.py:92-116), and what a rank transform starts from.
 *   dense_out[v]     = number of bins that hold v, for v < KDB_SPECTRUM_DENSE; exact uint64 (at k = 17 the entry of 0 passes 2^32)
 *   over_values_out  = every value >= KDB_SPECTRUM_DENSE, once per occurrence, in no particular order; *n_over_out of them
 * d_vector: nbins uint64 on device_id, 16-byte aligned, read only.  Synchronous; the caller has synchronised whatever produced the
 * vector; scratch is allocated and freed inside the call.  *n_over_out is always set; over_values_out may be NULL to ask for the
 * table and the number alone, otherwise it holds over_cap entries (KDB_ERR_ARG if fewer than *n_over_out, with *n_over_out and the
 * table set).  KDB_ERR_ARG: a NULL or misaligned pointer, nbins == 0 or above 2^36.  KDB_ERR_NOMEM: the scratch does not fit.
 * kernel_ms_out (may be NULL): device time of the sweep, by HIP events.
 * KDB_SPECTRUM_WG_BINS: bins one workgroup of either kernel covers per grid stride.  KDB_SPECTRUM_GRID_MAX: the most workgroups of
 * either kernel, so one grid stride is KDB_SPECTRUM_GRID_MAX x KDB_SPECTRUM_WG_BINS bins.  KDB_SPECTRUM_LIST_GUESS: the values
 * >= KDB_SPECTRUM_DENSE that kdb_rank_transform's first sweep has room for; a vector with more of them is swept a second time.
 */
#define KDB_SPECTRUM_DENSE 65536
#define KDB_SPECTRUM_WG_BINS 1024
#define KDB_SPECTRUM_GRID_MAX 1024
#define KDB_SPECTRUM_LIST_GUESS 1048576
int kdb_spectrum(int device_id, const void *d_vector, uint64_t nbins,
                 uint64_t *dense_out       /* KDB_SPECTRUM_DENSE words */,
                 uint64_t *over_values_out /* may be NULL */, uint64_t over_cap, uint64_t *n_over_out,
                 double   *kernel_ms_out   /* may be NULL */);

/*
 * The vector's doubled mid-ranks: d_ranks_out[b] = 2 #{c : x[c] < x[b]} + #{c : x[c] == x[b]} + 1 as uint64 -- twice what
 * scipy.stats.rankdata gives, an integer; Pearson's r of two such vectors is Spearman's rho of the counts (python_distances.py:95-114).
 * One spectrum sweep, the rank tables on the host (the list of large values is copied back, sorted and ranked there), one elementwise
 * sweep.  d_ranks_out: nbins uint64 on the same device, 16-byte aligned; it may be d_vector itself.  Conventions as above.
 * KDB_ERR_ARG also for nbins >= 2^32, before anything is read: the ranks sum to nbins (nbins + 1), which the moments of the ranks
 * need below 2^64.  kernel_ms_out (may be NULL): device time of both sweeps.
 */
int kdb_rank_transform(int device_id, const void *d_vector, uint64_t nbins, void *d_ranks_out /* may equal d_vector */,
                       double *kernel_ms_out);

/*
 * `counts = counts + counts_` over the files of a samplesheet (kmerdb/__init__.py:1888-1891) without leaving HBM.
 * kdb_fold_file: sync; add the engine's vector (one file's counts) to a second, engine-owned 4^k accumulator;
 * report that file's total_kmers / unique_kmers (its per-file metadata, parse.py:141-147); clear the file vector
 * and its totals for the next file -- one sweep.  kdb_finish_folded: copy the accumulator to `counts_out` (may be
 * NULL) and report its Sum / count_nonzero (__init__.py:1901-1902).  kdb_reset clears the accumulator too.
 * KDB_ERR_NOMEM if a second vector does not fit (k = 17): the host layer then sums on the host as before.
 */
int kdb_fold_file(kdb_engine *e, uint64_t *total_kmers, uint64_t *unique_kmers);
/* the same with the accumulator of ANOTHER engine (same k, same device): several engines count files at the same time
 * and fold into one sum; the caller serialises the folds into one accumulator (one at a time). */
int kdb_fold_file_into(kdb_engine *e, kdb_engine *acc, uint64_t *total_kmers, uint64_t *unique_kmers);
int kdb_finish_folded(kdb_engine *e, uint64_t *counts_out, uint64_t *total_kmers, uint64_t *unique_kmers);

/*
 * Device pointer of the count vector and its length 4^k (for the RCCL reduce by the host layer).  The vector
 * holds everything submitted so far only after kdb_sync / kdb_finish: submits are asynchronous, and for k >= 13
 * the histogram pass over scattered batches is deferred until then (see "defer_flush").
 */
int kdb_table(kdb_engine *e, void **d_table_out, uint64_t *nbins_out);

/* Error detail after KDB_ERR_SHORT_READ / KDB_ERR_BAD_RESIDUE: how many offenders were seen. */
int kdb_error_counts(kdb_engine *e, uint64_t *n_short_reads, uint64_t *n_bad_residues);

/*
 * An engine without a count vector, for kdb_shred / kdb_window_ids only (kmer.shred on single records must not
 * allocate 4^k * 8 bytes: 8 GiB at k = 15).  Counting entry points return KDB_ERR_STATE on it.  1 <= k <= 17.
 */
int kdb_create_ids(int k, int canonicalize, int device_id, kdb_engine **out);

/*
 * kmer.shred for one record on the device (kmer.py:489-577), N-free windows
 * only (n_mode is ignored: windows containing N emit nothing, as with
 * replace_with_none=True).  Writes one id per emitted window, in window order,
 * and its position.  ids_out/pos_out hold `cap` entries; *n_out is the number
 * of windows emitted (<= nbytes-k+1).
 */
int kdb_shred(kdb_engine *e, const uint8_t *seq, size_t nbytes,
              uint64_t *ids_out, uint64_t *pos_out, size_t cap, size_t *n_out);

/*
 * The id of the window starting at every residue position of a batch of records (the per-record lists
 * kmer.shred returns, kmer.py:573-577, laid out by position): ids_out[p] for p in [0, nbytes) is the k-mer id
 * of the window starting at residue p, or ~0 where no counted window starts (too close to the record's end,
 * or the window contains N).  Used by the De Bruijn edge list (graph.py:219-332).  Synchronous; nbytes <= 2^30.
 */
int kdb_window_ids(kdb_engine *e, const uint8_t *bases, size_t nbytes,
                   const uint64_t *read_offsets, size_t nreads, uint64_t *ids_out);

/*
 * Reads scored against a finished profile (csrc/kdb_score.hip.h): the reference's markov_probability, kmerdb/probability.py:36-151 --
 * the log-probability of a sequence under the (k-1)-order Markov chain the 4^k count vector defines -- for a batch of records, one
 * random 32-byte read of the vector per window instead of one index.read_line through a .kdbi file (probability.py:77-99).
 * With v the vector, a = pseudocount and total' = total + a 4^k, a window w is scored iff kdb_window_ids of a forward ids-engine emits an
 * id for it (whole inside its record, every residue ACGT), and then
 *   c(w) = v[id(w)] + a                (canonical != 0: v[min(id, rc(id))] + a, rc as in kdb_strand_merge)
 *   D(w) = Sum_{x in ACGT} c(prefix_{k-1}(w) x): on a forward profile the four bins 4 (id >> 2) .. + 3; at k = 1 the whole vector
 *   the first scored window of a record contributes ln c(w) - ln total' (the reference's px, probability.py:75), every later one
 *   ln c(w) - ln D(w) (its ast = qt / sum_qses, :91-99, :130-133); a window with c(w) == 0 contributes -inf (never nan).
 *   log10_p_out[r]      = (the sum of the record's terms) / ln 10; nan if the record has no scored window.  FLOAT: float64 natural logs
 *                         of integers converted once (D, up to 2^66, is formed in 128 bits and rounded to nearest even once), added in an
 *                         order fixed by the record's length and KDB_SCORE_PIECE alone: a record's outputs do not depend on the grid, on the
 *                         other records of the batch or on its place among them, and two calls return the same bits (on one build).
 *   windows_out[r]      = number of scored windows                                                     EXACT
 *   zero_windows_out[r] = number of scored windows whose bin v[...] is 0 (before the pseudocount)      EXACT
 *   min_count_out[r]    = the smallest v[...] over the scored windows, 2^64 - 1 if there are none      EXACT
 * d_vector: 4^k uint64 on device_id, 16-byte aligned, read only.  bases / read_offsets: host memory, as for kdb_window_ids, at most 2^30
 * residues per call.  Synchronous; the caller has synchronised whatever produced the vector; scratch is allocated and freed inside the call.
 * KDB_SCORE_CONTINUES: record 0 is the next piece of the previous call's last record: it starts with the last k-1 residues already given,
 * every one of its windows is a transition (no initial term) and it is exempt from the length check, as in kdb_submit_ex; the caller adds
 * the pieces' outputs.
 * KDB_SCORE_NONE_SCORED, with KDB_SCORE_CONTINUES only: none of the record's pieces so far held a scored window (N all along, or fewer
 * than k residues), so record 0's first scored window is the record's first and contributes the initial term ln c(w) - ln total'; the
 * exemption from the length check stays.  Without it such a record's first scored window would be weighed against D(w), which the
 * uncut record never does.  The caller knows: it adds the pieces' windows_out.
 * KDB_ERR_ARG: k outside 1..17, a NULL or misaligned pointer, total == 0, total + pseudocount 4^k or 4 pseudocount not below 2^64, offsets
 * that do not rise from 0 to nbytes, more than 2^30 residues, unknown flags, KDB_SCORE_NONE_SCORED without KDB_SCORE_CONTINUES.  KDB_ERR_SHORT_READ / KDB_ERR_BAD_RESIDUE: what kdb_window_ids
 * refuses (kmer.py:461-463; kmer.py:309 / :170), the outputs are then not written.  KDB_ERR_NOMEM: the scratch does not fit.
 * kernel_ms_out (may be NULL): device time of the residue check and the two scoring kernels, by HIP events.
 * KDB_SCORE_PIECE: windows one wave scores; a record of more windows is cut into pieces of that many, summed in piece order.
 * KDB_SCORE_LANES: lanes of the wave: a lane adds at most KDB_SCORE_PIECE / KDB_SCORE_LANES terms in a row before the log2(KDB_SCORE_LANES)
 * levels of the butterfly; every piece then adds two numbers to the record's sum.
 */
#define KDB_SCORE_CONTINUES 1
#define KDB_SCORE_NONE_SCORED 2
#define KDB_SCORE_PIECE 2048
#define KDB_SCORE_LANES 64
int kdb_score_reads(int device_id, const void *d_vector, int k, int canonical, uint64_t total, uint64_t pseudocount,
                    const uint8_t *bases, size_t nbytes, const uint64_t *read_offsets, size_t nreads, int flags,
                    double *log10_p_out, uint64_t *windows_out, uint64_t *zero_windows_out, uint64_t *min_count_out /* nreads each */,
                    double *kernel_ms_out /* may be NULL */);

/*
 * One small k-mer table per record (csrc/kdb_tables.hip.h): what the reference's codon tables are made of
 * (kmerdb/codons.py:175-333: k = 3, stride = 3, canonical ids) and, with stride 1, the composition vector of every record.
 * Record r holds the residues bases[off[r] .. off[r + 1]), len of them.  Its windows start at p_i = phase_r + i stride for every i >= 0
 * with p_i + k <= len; phase_r is 0, but for record 0 under KDB_TABLES_CONTINUES it is `phase`.  A window is COUNTED if its k residues
 * are all of A, C, G, T and SKIPPED if it holds an N (the frame is kept: codons.py:205-215).
 *   tables_out[r][id] = the number of counted windows with that id; id = the forward id, with canonical != 0 min(id, rc(id)), rc as in
 *                       kdb_strand_merge.  A row is 4^k entries wide either way.
 *   windows_out[r]    = the number of counted windows
 *   skipped_out[r]    = the number of skipped windows
 *   first_id_out[r] / last_id_out[r] = the id of the counted window with the smallest / largest p, -1 without one
 * All five are exact integers and do not depend on the grid, on the other records of the batch or on the record's place among them.
 * A record shorter than k, an empty one included, is no error: a row of zeros, 0, 0, -1, -1.
 * bases / read_offsets and all outputs: host memory.  Synchronous; scratch is allocated and freed inside the call.
 * KDB_TABLES_CONTINUES: record 0 is the next piece of the previous call's last record and begins with the last k - 1 residues already
 * given; phase (0 <= phase < stride) is where its first window starts, so that the record's windows keep their frame.  The caller works
 * it out (the length and first phase of the piece before fix where the next window of the record starts) and joins the pieces: rows and
 * counts added, the first first_id that is not -1, the last last_id that is not -1.
 * KDB_ERR_ARG, all settled on the host before anything is launched: k outside 1..6 (4^6 uint32 are the 16 KiB of LDS one wave owns),
 * stride outside 1..k, phase >= stride, phase != 0 without the flag, unknown flags, a NULL buffer, offsets that do not start at 0, end at
 * nbytes and rise, more than 2^30 residues or records, nreads 4^k above 2^31 table entries, residues but no records.  No records and no
 * residues: KDB_OK.
 * KDB_ERR_BAD_RESIDUE: a byte outside upper-case ACGTN anywhere in the batch; the outputs are then not written.  This is one step
 * stricter than the reference, which never looks at the letters of a triplet that holds an N (codons.py:205-215) and so lets an IUPAC
 * letter beside an N pass.
 * KDB_ERR_NOMEM: the scratch does not fit.  kernel_ms_out (may be NULL): device time of the kernels, by HIP events.
 * KDB_TABLES_PIECE: windows one wave counts; a record of more windows is cut into pieces of that many, whose rows are added.
 */
#define KDB_TABLES_CONTINUES 1
#define KDB_TABLES_PIECE 8192
#define KDB_TABLES_MAX_K 6
int kdb_record_tables(int device_id, int k, int stride, int canonical, uint64_t phase,
                      const uint8_t *bases, size_t nbytes, const uint64_t *read_offsets, size_t nreads, int flags,
                      uint32_t *tables_out /* nreads x 4^k, row-major */,
                      uint64_t *windows_out, uint64_t *skipped_out, int32_t *first_id_out, int32_t *last_id_out /* nreads each */,
                      double *kernel_ms_out /* may be NULL */);

/*
 * The (w,k)-minimizers of every record (csrc/kdb_minimizers.hip.h): the sketch that read mappers, containment
 * estimates and index subsampling start from.  The reference's `minimizers` subcommand (kmerdb/minimizer.py) flags every window_size-th
 * of 4^k - k + 1 positions, which is no minimizer scheme; this call computes the usual one.
 * Record r holds the residues bases[off[r] .. off[r + 1]), len of them.  Its start positions are 0 .. nwin - 1 with nwin = len - k + 1
 * (0 if len < k).  Position p has an id iff kdb_window_ids of a forward ids-engine emits one for it (the window lies whole inside the
 * record and every residue is one of A, C, G, T); fwd(p) is that id, rc as in kdb_strand_merge, and
 *   id(p)     = canonical ? min(fwd, rc(fwd)) : fwd
 *   strand(p) = 1 iff canonical and rc(fwd) < fwd, else 0
 *   key(p)    = id(p) under KDB_MINIMIZER_LEX; under KDB_MINIMIZER_HASHED h(id(p)) with m = 4^k - 1 and every step masked:
 *                 x = (~x + (x << 21)) & m;  x ^= x >> 24;  x = (x + (x << 3) + (x << 8)) & m;  x ^= x >> 14;
 *                 x = (x + (x << 2) + (x << 4)) & m;  x ^= x >> 28;  x = (x + (x << 31)) & m;
 *               (a bijection of [0, 4^k): equal keys mean equal ids).  A position without an id has key +infinity.
 * With we = min(w, nwin): for every run of we consecutive start positions s .. s + we - 1, 0 <= s <= nwin - we, whose smallest key is
 * finite, the LEFTMOST position holding that key is selected.  A record's minimizers are its selected positions, each once, ascending.
 * A record with 1 <= nwin < w is one run; one with nwin = 0 or no finite key has none, which is no error.
 *   counts_out[r] = the number of minimizers of record r; S_r = counts_out[0] + .. + counts_out[r - 1]
 *   ids_out / pos_out / strand_out [S_r .. S_r + counts_out[r]) = id(p), p and strand(p) of record r's minimizers, by position
 *   *total_out    = the sum of the counts
 * All are exact integers and do not depend on the grid, on the other records of the batch or on the record's place among them.
 * counts_out and *total_out are written whenever the status is KDB_OK.  The flat arrays hold `cap` entries and are written only if
 * *total_out <= cap; otherwise they are left as they were and the status is still KDB_OK: the caller compares and calls again with room.
 * cap == 0 with NULL flat pointers asks for the sizes alone.  strand_out may be NULL whatever cap is.
 * bases / read_offsets and all outputs: host memory.  Synchronous; scratch is allocated and freed inside the call.
 * KDB_ERR_ARG, all settled on the host before anything is launched: k outside 1..KDB_MINIMIZER_MAX_K (keys and ids in 64 bits), w outside
 * 1..KDB_MINIMIZER_MAX_W, an order that is neither of the two, NULL counts_out, total_out or offsets, NULL ids_out or pos_out with
 * cap > 0, offsets that do not start at 0, end at nbytes and rise, more than 2^30 residues or records, residues but no records.  No
 * records and no residues: KDB_OK, *total_out = 0.
 * KDB_ERR_BAD_RESIDUE: a byte outside upper-case ACGTN anywhere in the batch; no output is written (as kdb_record_tables).
 * KDB_ERR_NOMEM: the scratch does not fit.  kernel_ms_out (may be NULL): device time of the kernels, by HIP events.
 * KDB_MINIMIZER_PIECE: start positions one wave owns; a record of more is cut into pieces of that many, each of which reads the keys of
 * w - 1 positions on either side and so decides its own positions alone.
 */
#define KDB_MINIMIZER_LEX     0
#define KDB_MINIMIZER_HASHED  1
#define KDB_MINIMIZER_MAX_K   31
#define KDB_MINIMIZER_MAX_W   256
#define KDB_MINIMIZER_PIECE   2048
int kdb_minimizers(int device_id, int k, int w, int canonical, int order,
                   const uint8_t *bases, size_t nbytes, const uint64_t *read_offsets, size_t nreads,
                   uint64_t *counts_out /* nreads */,
                   uint64_t *ids_out, uint32_t *pos_out, uint8_t *strand_out /* may be NULL */, size_t cap,
                   uint64_t *total_out,
                   double *kernel_ms_out /* may be NULL */);

/*
 * A batch of independent banded local alignments with affine gaps (csrc/kdb_align.hip.h): the extend step of
 * seed-and-extend, for the seeds kdb_minimizers gives.  Per task the score and the four end coordinates; the path between them, as
 * CIGAR runs, is kdb_align_traceback's, below.
 * The reference's `alignment` subcommand (kmerdb/__init__.py:454-573) exits before it aligns; its score arguments are kept, nothing else.
 * Query record x is q_bases[q_offsets[x] .. q_offsets[x + 1]), reference record y likewise in r_bases.  Task t aligns query task_q[t] to
 * reference task_r[t]:
 *   Q = the oriented query of length m: strand 0 the record q itself; strand 1 its reverse complement, Q[i] = comp(q[m - 1 - i]), N stays N
 *   R = the reference record of length n;  d = task_diag[t]
 *   cell (i, j), 0 <= i < m, 0 <= j < n, is IN BAND iff |(j - i) - d| <= band
 *   s(i, j) = match if Q[i] = R[j] and both are one of A, C, G, T, else mismatch (an N matches nothing, not even an N)
 *   anything not in band, or with a negative index, counts as -infinity for E and F and as 0 for H; over the in-band cells
 *     E(i, j) = max(H(i, j - 1) + gap_open, E(i, j - 1) + gap_extend)
 *     F(i, j) = max(H(i - 1, j) + gap_open, F(i - 1, j) + gap_extend)
 *     H(i, j) = max(0, H(i - 1, j - 1) + s(i, j), E(i, j), F(i, j))          (gap_open is the cost of a gap's first residue)
 *   ORIGINS: every finite H, E and F carries the cell where its alignment starts.  A cell whose H takes the diagonal term from a predecessor
 *     with H = 0, or from no predecessor, starts at (i, j); the diagonal term otherwise inherits its predecessor's origin.  E and F inherit
 *     the origin of the term that wins, the H + gap_open term on a tie.  H takes the origin of the first of [diagonal, E, F] that reaches
 *     its value.  H = 0 has no origin.
 *   BEST CELL: the largest H; on a tie the smallest i, then the smallest j.
 *   score_out[t] = that H; qend_out[t] = i + 1, rend_out[t] = j + 1; (qstart_out[t], rstart_out[t]) = its origin.  Query coordinates are
 *     those of the oriented query Q.  If no cell scores above 0 -- a band that misses the record, an empty record -- the score and all four
 *     coordinates are 0, which is no error.
 * All are exact integers and do not depend on the grid, on the other tasks or on the task's place among them.
 * Limits: 1 <= band <= KDB_ALIGN_MAX_BAND; 1 <= match <= 127; -127 <= mismatch, gap_open, gap_extend <= 0; a query record holds at most
 * KDB_ALIGN_MAX_QUERY = 2^20 residues (a score stays below 2^27); at most 2^30 residues per buffer and 2^26 tasks.
 * All pointers: host memory.  Synchronous; scratch is allocated and freed inside the call.
 * KDB_ERR_ARG, all settled on the host before anything is launched: a limit above, a NULL pointer (a residue buffer of 0 bytes may be
 * NULL), offsets that do not start at 0, end at the buffer's size and rise, a task index that names no record, a strand above 1.
 * KDB_ERR_BAD_RESIDUE: a byte outside upper-case ACGTN in either buffer; no output is written (as kdb_minimizers).
 * KDB_ERR_NOMEM: the scratch does not fit.  ntasks = 0: KDB_OK once the scalars are in range.  kernel_ms_out (may be NULL): device time
 * of the kernel, by HIP events.
 * KDB_ALIGN_STAGE: the anti-diagonal steps a wave takes between two refills of its residues in LDS; KDB_ALIGN_GRID_MAX: the most
 * workgroups of a launch, 4 tasks under way in each.
 */
#define KDB_ALIGN_MAX_BAND   63
#define KDB_ALIGN_MAX_QUERY  1048576
#define KDB_ALIGN_STAGE      512
#define KDB_ALIGN_GRID_MAX   4096
int kdb_align_banded(int device_id,
                     const uint8_t *q_bases, size_t q_nbytes, const uint64_t *q_offsets, size_t nq,
                     const uint8_t *r_bases, size_t r_nbytes, const uint64_t *r_offsets, size_t nr,
                     const uint32_t *task_q, const uint32_t *task_r, const int64_t *task_diag, const uint8_t *task_strand, size_t ntasks,
                     int band, int match, int mismatch, int gap_open, int gap_extend,
                     int32_t *score_out, uint32_t *qstart_out, uint32_t *qend_out, uint32_t *rstart_out, uint32_t *rend_out /* ntasks each */,
                     double *kernel_ms_out /* may be NULL */);

/*
 * The same batch of alignments with their paths (csrc/kdb_align_trace.hip.h): what kdb_align_banded reports and, per
 * task, the run-length encoded alignment from the origin to the best cell.  The records, the tasks, band and the scores are
 * kdb_align_banded's, and so is everything in its comment: oriented query, band, s(i, j), H / E / F, tie rules, best cell.  The five
 * scalar outputs are bit-equal to kdb_align_banded's on the same arguments.
 * THE TRACEBACK is the walk those tie rules imply.  Start at the best cell in state H.
 *   state H at (i, j): if H took the diagonal term (the first of [diagonal, E, F] that reaches its value): emit `=` if Q[i] = R[j] and both
 *     are one of A, C, G, T, else `X`; if H(i - 1, j - 1) = 0, or there is no such cell, stop; otherwise continue in state H at
 *     (i - 1, j - 1).  If H took E: go to state E at (i, j) and emit nothing.  Otherwise go to state F at (i, j) and emit nothing.
 *   state E at (i, j): emit `D` (R[j] is against a gap).  If H(i, j - 1) + gap_open >= E(i, j - 1) + gap_extend continue in state H at
 *     (i, j - 1), otherwise in state E at (i, j - 1).
 *   state F at (i, j): emit `I`.  If H(i - 1, j) + gap_open >= F(i - 1, j) + gap_extend continue in state H at (i - 1, j), otherwise in
 *     state F at (i - 1, j).
 * The emitted ops are reversed and run-length encoded; equal neighbours merge (two separate gaps of one kind can only abut where
 * gap_open > gap_extend, and then read as one run).  A run is one uint32, (len << 4) | op, with BAM's op codes I = 1, D = 2, `=` = 7,
 * X = 8.  A task without a positive score has no runs.  What follows from the definition: the walk stops exactly at the origin
 * (qstart, rstart); the runs consume qend - qstart query residues (=, X, I) and rend - rstart reference residues (=, X, D); match per =,
 * mismatch per X and gap_open + (len - 1) max(gap_open, gap_extend) per gap run add up to the score; a task has at most
 * (qend - qstart) + (rend - rstart) runs.
 * nruns_out[t]: the runs of task t; they are runs_out[S_t .. S_t + nruns_out[t]), S the exclusive prefix sums of nruns_out, in alignment
 * order from the origin to the end cell.  The cap protocol is kdb_minimizers': the five scalars, nruns_out and *total_out (the sum of
 * nruns_out) are written whenever the status is KDB_OK; runs_out, which holds cap entries, only if *total_out <= cap; cap = 0 with
 * runs_out = NULL asks for the sizes alone.
 * All are exact integers and do not depend on the grid, on the other tasks, on the task's place among them or on scratch_limit.
 * SCRATCH: the forward pass leaves 4 bits per cell -- where H came from (2 bits) and whether the E and the F the cell hands on opened or
 * extended --, 64 bytes per anti-diagonal step of a task whatever the band, in whole groups of 4 steps: about 11 KB for 150 residues at
 * band 16, 67 MB for 2^20.  The call works through its tasks in chunks of consecutive tasks: a chunk is the longest run of tasks whose
 * directions fit scratch_limit bytes (0: KDB_ALIGN_TRACE_SCRATCH, 2 GiB -- a choice, not a measurement) and holds at least one task.
 * Limits and errors as kdb_align_banded, all settled on the host before anything is launched, and no output is written on a refusal;
 * also KDB_ERR_ARG: nruns_out or total_out NULL, runs_out NULL where cap > 0.  KDB_ERR_NOMEM: the scratch -- the largest chunk's
 * directions, cap runs -- does not fit.  ntasks = 0: KDB_OK and *total_out = 0 once the scalars are in range.  kernel_ms_out (may be
 * NULL): device time of all kernels of all chunks, by HIP events.
 */
#define KDB_ALIGN_TRACE_SCRATCH 2147483648ull
int kdb_align_traceback(int device_id,
                        const uint8_t *q_bases, size_t q_nbytes, const uint64_t *q_offsets, size_t nq,
                        const uint8_t *r_bases, size_t r_nbytes, const uint64_t *r_offsets, size_t nr,
                        const uint32_t *task_q, const uint32_t *task_r, const int64_t *task_diag, const uint8_t *task_strand, size_t ntasks,
                        int band, int match, int mismatch, int gap_open, int gap_extend,
                        size_t scratch_limit,
                        int32_t *score_out, uint32_t *qstart_out, uint32_t *qend_out, uint32_t *rstart_out, uint32_t *rend_out /* ntasks each */,
                        uint64_t *nruns_out /* ntasks */, uint32_t *runs_out, size_t cap, uint64_t *total_out,
                        double *kernel_ms_out /* may be NULL */);

/*
 * Host-side record splitter (no GPU work): what Bio.SeqIO.parse does for kmerdb/parse.py:50-85 on this path.
 * FASTQ: parses whole records of text[0, n) into bases_out (concatenated residues) and offsets_out
 * (nreads+1 entries); *consumed_out = bytes of text used (stops before a trailing partial record unless at_eof).
 * The usual four-line records take the fast path; a text that is not of that form goes through the general grammar of
 * Bio.SeqIO's FASTQ reader (sequence and quality wrapped over several lines, a '+' line that repeats the title, quality
 * lines that start with '@'), and, like that reader, a quality character outside 33..126, differing sequence and quality
 * lengths or captions are malformed input.  kdb_parse_fastq_mt: the same on `nthreads` threads (the text is cut at record
 * starts, every piece is counted, then split into its final place; same outputs, same errors).
 * FASTA: the whole text; sequence lines are concatenated, blanks / CR dropped, text before the first '>' ignored.
 * header_spans_out (optional, 2 per record) = [start, end) of each header line in `text` (for record ids).
 * Malformed input -> KDB_ERR_ARG (the host layer raises ValueError).
 */
int kdb_parse_fastq(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap,
                    uint64_t *offsets_out, size_t cap_reads, uint64_t *header_spans_out,
                    size_t *nreads_out, size_t *nbases_out, size_t *consumed_out);
int kdb_parse_fastq_mt(const uint8_t *text, size_t n, int at_eof, uint8_t *bases_out, size_t bases_cap,
                       uint64_t *offsets_out, size_t cap_reads, uint64_t *header_spans_out,
                       size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int nthreads);
int kdb_parse_fasta(const uint8_t *text, size_t n, uint8_t *bases_out, size_t bases_cap,
                    uint64_t *offsets_out, size_t cap_reads, uint64_t *header_spans_out,
                    size_t *nreads_out, size_t *nbases_out);

/*
 * kdb_parse_fasta for a file read in chunks: in_record = the chunk starts inside a record (then record 0 of the output
 * is that record's next piece; 2 = in the middle of one of its lines); header lines are consumed whole, sequence text as far as it goes;
 * *in_record_out = the state to pass with the next chunk.
 */
int kdb_parse_fasta_chunk(const uint8_t *text, size_t n, int at_eof, int in_record, uint8_t *bases_out, size_t bases_cap,
                          uint64_t *offsets_out, size_t cap_reads, uint64_t *header_spans_out,
                          size_t *nreads_out, size_t *nbases_out, size_t *consumed_out, int *in_record_out);

/*
 * Block-parallel inflate of BGZF input (bgzip / Bio.bgzf files; what the reference reads through gzip.open,
 * kmerdb/parse.py:64-72): inflates the whole BGZF members of src[0, n) that fit `cap` with `nthreads` threads, checks
 * their CRC32.  *consumed_out = input bytes used (stops before an incomplete member), *produced_out = bytes written.
 * KDB_ERR_ARG if the input is not BGZF or is corrupt.
 */
int kdb_bgzf_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int nthreads,
                     size_t *consumed_out, size_t *produced_out);

/*
 * Index of a BGZF file from its members' headers and trailers (nothing is inflated): coff_out[i] / uoff_out[i] =
 * compressed / uncompressed offset of member i, entry n = the file's sizes; *n_out = n + 1 entries.  With it a rank of
 * a multi-GPU job inflates only the members that hold the blocks it owns (the reference reads the whole file through
 * gzip.open on its one process, kmerdb/parse.py:64-72).  KDB_ERR_ARG if the file is not BGZF; KDB_ERR_NOMEM if `cap`
 * entries do not hold the index (call again with more).
 */
int kdb_bgzf_scan(const char *path, uint64_t *coff_out, uint64_t *uoff_out, size_t cap, size_t *n_out);

/*
 * One gzip stream -- what the reference opens with gzip.open (kmerdb/parse.py:64-72) -- inflated by a thread of its
 * own into a ring of 4 MiB buffers, ahead of the reader: inflating overlaps record splitting, hashing and counting.
 * kdb_gz_read fills `dst` with up to `cap` bytes (fewer only at the end of the stream; 0 = end); concatenated members
 * are concatenated output.  KDB_ERR_ARG for a file that cannot be opened or a corrupt / truncated stream.
 */
typedef struct kdb_gz kdb_gz;
int kdb_gz_open(const char *path, kdb_gz **out);
int kdb_gz_read(kdb_gz *g, uint8_t *dst, size_t cap, size_t *n_out);
int kdb_gz_close(kdb_gz *g);

/*
 * Host-side .kdb row writer (no GPU work): the per-row loop kmerdb/__init__.py:1980-1990 plus
 * Bio.bgzf.BgzfWriter._write_block.  Appends to `path` (which already holds the YAML header member written by
 * the host layer) the rows "{i}\t{i}\t{count}\t{count/total}\n", i = 0..nbins-1, as BGZF members of exactly
 * 65536 uncompressed bytes (last one partial, no EOF marker -- like the reference).  The frequency is printed as
 * Python prints numpy.float64 (shortest round-trip repr).  kdb_format_frequency exposes that formatter.
 */
int kdb_write_kdb_rows(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers,
                       int compresslevel, int nthreads, uint64_t *nblocks_out);
/*
 * The same with the deflate encoder named.  KDB_ENCODER_ROWS (what KDB_ENCODER_DEFAULT means unless the environment says
 * KDB_KDB_ENCODER=zlib): the row-aware encoder -- the text's own structure says where its repeats are (an id's leading
 * digits in the row before, the second id column in the first, a row's "count \t frequency \n" string in the last row with
 * that count), so LZ77 needs no search; one dynamic-Huffman block per member; `compresslevel` is not used.  About ten times
 * zlib level 6 per thread at a slightly better ratio.  KDB_ENCODER_ZLIB: zlib at `compresslevel`, what Bio.bgzf does for the
 * reference.  Either way the decompressed stream and the member boundaries are the reference's; the compressed bytes are not
 * comparable between encoders (nor between zlib versions).
 */
#define KDB_ENCODER_DEFAULT (-1)
#define KDB_ENCODER_ROWS      0
#define KDB_ENCODER_ZLIB      1
int kdb_write_kdb_rows_ex(const char *path, const uint64_t *counts, uint64_t nbins, uint64_t total_kmers,
                          int compresslevel, int nthreads, int encoder, uint64_t *nblocks_out);
int kdb_format_frequency(uint64_t count, uint64_t total, char *buf, size_t cap);
/*
 * kdb_finish's copy-back and kdb_write_kdb_rows_ex in one: the count vector (`folded` = 1: the samplesheet accumulator) comes back into
 * `counts_out` (4^k uint64, caller-owned) in pieces while the writer's threads are already formatting and deflating the rows that have
 * arrived -- the writer needs a chunk's own counts only, never the whole vector first.  Syncs the engine; the caller has the totals
 * (kdb_finish / kdb_finish_folded with counts_out = NULL) and has written the header member(s) to `path` before.  At k = 15 the 0.2 s of
 * the 8 GiB copy-back disappear under the 1.7 s of the rows.
 */
int kdb_copy_back_and_write_kdb_rows(kdb_engine *e, int folded, uint64_t *counts_out, const char *path, uint64_t total_kmers,
                                     int compresslevel, int nthreads, int encoder, uint64_t *nblocks_out);
/*
 * The way back (no GPU work): KDBReader._slurp, kmerdb/fileutil.py:308-466, reads the 4^k rows one by one through Bio.bgzf.  Here the
 * file's BGZF members are inflated in groups on `nthreads` threads and parsed where they were inflated.  Row "x \t kmer_id \t count \t f":
 * kmer_ids_out[x] = kmer_id, counts_out[kmer_id] = count, frequencies_out[kmer_id] = f (the file's column); x must be the row's line number
 * and there must be exactly `nbins` rows of four columns behind the header's delimiter line, else KDB_ERR_ARG.  The arrays hold `nbins`
 * entries each (zero them first: the reference's arrays start as zeros).  KDB_ERR_STATE: the file is not a sequence of BGZF members (one
 * plain gzip stream, say): the host layer reads it through gzip instead.
 */
int kdb_read_kdb_rows(const char *path, uint64_t nbins, uint64_t *kmer_ids_out, uint64_t *counts_out, double *frequencies_out,
                      int nthreads, uint64_t *nrows_out);

/*
 * Per-kernel timing with HIP events on the engine's compute stream (the stream
 * the kernels are launched on).  Enable, run submits, sync, then read back the
 * accumulated device time and launch count of each kernel.
 * kernel ids: see KDB_KERNEL_* ; name via kdb_prof_kernel_name.
 */
#define KDB_KERNEL_MARK          0   /* lens_kernel + hibit_check_kernel + mark_reads_kernel: record geometry, checks, start marks */
#define KDB_KERNEL_COUNT         1   /* count_direct_kernel (global atomics), count_lds_kernel (k <= 7), expand_worklist_kernel */
#define KDB_KERNEL_SCATTER       2   /* scatter_bases_kernel: residues -> pages of bins (k <= 12) or of remainders (level 1, k >= 13) */
#define KDB_KERNEL_SCATTER_L2    3   /* scatter_ids_kernel: level-1 pages -> pages of bins (k >= 13) */
#define KDB_KERNEL_PAGE_SORT     4   /* pages_count / pages_scan / pages_place (+ l2_plan): page tags -> one page list per bucket */
#define KDB_KERNEL_PAGE_HIST     5   /* page_hist_kernel: one 32768-bin LDS histogram per bucket, added to the vector */
#define KDB_KERNEL_STATS         6   /* stats_kernel / fold_kernel: count_nonzero, Sum, samplesheet accumulation */
#define KDB_KERNEL_STRAND_MERGE   7   /* strand_merge_kernel: forward counts of a canonical engine -> canonical bins of the vector, once per sync */
#define KDB_N_KERNELS            8
int         kdb_prof_enable(kdb_engine *e, int on);
int         kdb_prof_reset(kdb_engine *e);
int         kdb_prof_get(kdb_engine *e, int kernel_id, double *total_ms, uint64_t *launches);
const char *kdb_prof_kernel_name(int kernel_id);

/*
 * Tuning knobs (ints); unknown names return KDB_ERR_ARG.
 *   set: "algo" 0 auto / 1 direct global atomics / 2 LDS-histogram paths (k <= 7 whole vector in LDS, else paged scatter);
 *        "defer_flush" 1/0 (k >= 13: add the scattered batches to the vector together -- at kdb_sync, after 64 batches or
 *        when the page arena is full -- instead of after every batch);  "pending_budget" (bytes the page arena may grow
 *        to; 0 = decide at first use: 85 % of the free device memory, at most 192 GiB);  "reserve_bytes" (device memory the arena
 *        must leave free when it sizes itself -- for what is allocated later beside it: RCCL's buffers at the first collective of each
 *        kind and the scratch of the end-of-job reduce, kmerdb_amd.distributed.reduce_reserve_bytes);  "arena_grow" (the arena starts with
 *        room for eight batches; 0: it stays that size, 1 (default): it doubles once the vector sweeps a larger one would have
 *        saved outweigh the allocation -- fresh device memory costs ~46 ms per GiB --, 2: it doubles whenever it has filled
 *        up: long-lived engines, benchmarks of the steady state);  "arena_batches" (1..64: room for that many batches
 *        like the first one instead of eight -- one allocation instead of a doubling series);  "sc_grid" (persistent
 *        workgroups of the scatter kernels);  "sc_top_bits" 1/0 (k <= 12: buckets from the leading id bits; diagnostic);
 *        "min_len";  "copy_threads", "accum_bytes" (-1 auto: 1 GiB for k >= 13), "stage_bytes", "stage_reads" (host staging);
 *        "one_level_max_k" 13/12 (k = 13 in one scatter level with 1024 rings, or through the two-level path);  "smallk_old" 0/1
 *        (k <= 8 in one CU's LDS, or as before round 4: k <= 7 count_lds_kernel, k = 8 paged scatter);  "overlap" 0/1 (one-level path,
 *        DROP mode: the scatter kernel of batch i + 1 on the compute stream beside the histogram pass of batch i on a second stream;
 *        off by default -- measured slower), "overlap_hist_cus" (> 0: the two streams get disjoint CU masks, that
 *        many CUs for the pass; a diagnostic that needs KDB_ALLOW_CU_MASKS=1 in the environment: on ROCm 7.2 a process that has created a
 *        CU-masked stream crashes or hangs in the runtime when a later hipMalloc runs out of memory), "overlap_mask_mode" (which CUs: 0 the
 *        first, 1 every n-th, 2 the first of every 32);  "sc_wide_lines" / "l1_wide_lines" / "l2_wide_lines" 1/0 (default 1: the scatter kernels of
 *        k <= 12 / level 1 / level 2 write their pages in 128-byte pieces, one workgroup of 1024 threads per CU; 0: 64-byte lines, two
 *        workgroups of 512 -- the form of rounds 2-4, kept for comparison: the memory system takes random 64-byte writes at 3.4-4.6 TB/s
 *        and 128-byte ones at 5.3);  "l1_compiled_k" 1/0 (k = 15: level 1 / level 2 with their shifts compiled in);
 *        "l1_one_round" 1/0 (default 1: level 1 of k <= 15 with 128 rings of 256 elements -- one placement round per tile -- instead of 256 of 128).
 *        "strand_merge" 1/0 (default 1: a canonical engine's batches of the one-level paths -- k <= 8 in LDS, k = 9..12 through one scatter
 *        level -- count FORWARD ids into a staging vector of the engine's own, 4^k uint64 allocated at the first such batch, and kdb_sync adds
 *        both strands to the count vector at the canonical bins, kdb_strand_merge; 0: min(forward, reverse complement) per window in the
 *        counting kernels.  The vector a caller reads after a sync is the same either way; it is not written between syncs when the option
 *        is on.  Not used with "overlap" or "smallk_old", nor when the staging vector cannot be allocated),  "strand_merge_max_k" (1..17,
 *        default 12: the largest k that is staged; 13 stages k = 13's one-level path too -- 512 MiB, measured no faster --, and the two-level
 *        paths, k > "one_level_max_k", never are).  Setting either syncs first.
 *        "one_level_defer" -1 / 0 / 2..64 (the one-level path, k = 9 .. "one_level_max_k": 0 sorts a batch's pages and adds them to the
 *        vector right behind its scatter kernel; N keeps up to N scattered batches in a page arena -- about 2.05 bytes per residue of a
 *        batch, within "pending_budget" / "reserve_bytes" like the arena of k >= 13 -- and adds them with one sort and one histogram pass:
 *        when N are pending, when the next batch does not fit, and at kdb_sync; -1 (default): 4 for k <= 12, 0 for k = 13.  The vector
 *        after a sync is the same either way, and as with "strand_merge" it is not written between syncs.  Where not even two batches fit,
 *        batches are counted as with 0.  Not used with "overlap" or "algo" 1.  Setting it adds what is pending first.)
 *        The environment variable KDB_ENGINE_OPTS="name=value,..." sets options for every engine a process creates (experiments, the test
 *        suite under an option); an unknown name fails kdb_create.
 *   get: "sc_wide_lines", "l1_wide_lines", "l2_wide_lines", "l1_one_round", "reserve_bytes", "arena_budget_bytes" (what the arena may grow to, once decided), "free_at_sizing" (free device memory when it
 *        was decided), "free_hbm" (free device memory now), "overlap", "overlap_hist_cus", "overlap_scatter_grid",
 *        "algo", "stage_bytes", "stage_reads", "defer_flush", "k", "oom_fallbacks" (batches counted by direct atomics
 *        because scratch did not fit), "pending_batches" (scattered batches not yet added to the vector), "d2h_bytes"
 *        (bytes of count vector copied to the host so far), "folded_files", "sc_lo_bits", "sc_contig_pages", "arena_grow",
 *        "arena_batches", "arena_pages" / "arena_reallocs" (size of the page arena in 1 KiB pages; times it was (re)allocated),
 *        "arena_cursor" / "arena_used_bound" / "arena_worst_case" (pages the pending batches hold: on the device, by the host's
 *        present bound, and by their worst cases added up), "one_level_max_k", "smallk_old", "strand_merge", "strand_merge_max_k",
 *        "hist_flushes" / "flushed_batches" / "full_flushes" (k >= 13, and "one_level_defer": histogram passes over the arena, the batches
 *        they added to the vector, and how many of the passes a full arena forced), "one_level_defer", "one_level_pending" (batches the deferred
 *        one-level path has scattered but not yet added; "pending_batches" counts those of k >= 13), "arena_region_base" (the arena page
 *        at which the region of the next batch of the deferred one-level path would begin; 0: none pending), "bytes_in" and the
 *        device counters "pages_bases", "lines_bases", "pages_ids", "lines_ids", "table_bytes", "total_kmers" (what the
 *        kernels moved since kdb_reset, by their own count; reading one synchronises the compute stream).
 */
/*
 * Diagnostic (bench.py: `roofline.pattern_ceilings`): what the memory system of the device delivers for the access patterns of the engine's kernels
 * with NO compute -- streamed residues in, random 64-byte lines / 128-byte pieces out, whole pages in (csrc/kdb_probe.hip.h;
 * tools/ubench_hbm_pattern.hip prints the full table).  Runs every pattern (kdb_hbm_pattern_count of them, named by kdb_hbm_pattern_name) for a few
 * milliseconds on two scratch regions of 4 GiB and returns GB/s (read + written) per pattern.  Nothing of the reference corresponds to it.
 */
int         kdb_hbm_pattern_count(void);
const char *kdb_hbm_pattern_name(int i);
int         kdb_hbm_pattern_probe(int device_id, double *gb_per_s_out, int n_out);
int kdb_set_option(kdb_engine *e, const char *name, int64_t value);
int kdb_get_option(kdb_engine *e, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* KDBHIP_H */
