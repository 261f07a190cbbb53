/*
 * lbf_hash.h -- C ABI of the MI355X chunk-hash path for bitflood.
 *
 * This is the drop-in boundary beneath the reference's C++ entry points
 *   Error::ErrorCode libBitFlood::Encoder::Base64Encode(const U8*, U32, std::string&)
 *       (/root/reference/cpp/src/Encoder.H:28, Encoder.cpp:107-120)
 *   Error::ErrorCode libBitFlood::Encoder::EncodeFile(const ToEncode&, FloodFile&)
 *       (/root/reference/cpp/src/Encoder.H:27, Encoder.cpp:17-102)
 * and beneath the verify call sites that compare a chunk's hash with the
 * flood-file string
 *   Flood::_SetupFilesAndChunks      (/root/reference/cpp/src/Flood.cpp:259-275)
 *   ChunkMethodHandler::_HandleRequestChunk (/root/reference/cpp/src/ChunkMethods.cpp:116-123)
 *   ChunkMethodHandler::_HandleSendChunk    (/root/reference/cpp/src/ChunkMethods.cpp:165-167)
 * The C++ wrappers with the reference's exact signatures live in
 * include/libBitFlood/ (libbitflood.so); they call only what is declared here.
 *
 * Conventions (C convention, unlike the reference's ErrorCode where 1 = ok):
 *   - every int-returning call returns LBF_OK (0) on success or a negative
 *     lbf_status; lbf_last_error() returns a thread-local message;
 *   - the caller owns every host array; a context owns device memory,
 *     streams and pinned staging;
 *   - digests are raw 20-byte SHA-1 (big-endian word order, as the reference's
 *     HashFilter emits them, iterhash.h:117-118); chunk i's digest is at
 *     out_digests + 20*i;
 *   - nothing is thrown across the ABI.
 */
#ifndef LBF_HASH_H_
#define LBF_HASH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBF_ABI_VERSION 1
#define LBF_DIGEST_BYTES 20
#define LBF_B64_CHARS 27

typedef enum lbf_status {
  LBF_OK = 0,
  LBF_ERR_INVALID = -1,   /* bad argument (null pointer, size overflow, ...) */
  LBF_ERR_NO_DEVICE = -2, /* no MI355X visible: the path has no CPU fallback */
  LBF_ERR_HIP = -3,       /* HIP runtime or kernel launch failure */
  LBF_ERR_NOMEM = -4,     /* device or pinned host allocation failed */
  LBF_ERR_IO = -5         /* file could not be opened / read */
} lbf_status;

/* `flags` for the batch calls: where `base`, `offsets`, `sizes`, `expected`
 * and the outputs live. */
#define LBF_HOST_PTR 0
#define LBF_DEVICE_PTR 1

typedef struct lbf_ctx lbf_ctx;

/* ---- library / context ------------------------------------------------- */
int lbf_abi_version(void);
const char* lbf_last_error(void);
/* Number of visible GPUs (0 when none; never an error on a CPU-only host). */
int lbf_device_count(int* out_count);
/* device_mask bit d selects device d; 0 selects every visible device.
 * Fails with LBF_ERR_NO_DEVICE when no GPU is visible.  Host-path staging,
 * read at creation: batches of up to LBF_SLOT_MB MiB (default 512) in HBM
 * device slots (as many as one chain's duration at PCIe rate needs, within
 * LBF_DEVICE_STAGING_MB, default 16384), fed through LBF_SLOTS pinned host
 * slots per worker (2..8, default 3) of up to LBF_PIN_MB MiB (default 128),
 * all grown on demand; LBF_COPY_THREADS host copy threads (default 8).  Pinned staging is allocated on the GPU's NUMA node and
 * the copy threads run on that node's CPUs (LBF_NUMA=0 turns this off). */
int lbf_ctx_create(uint32_t device_mask, lbf_ctx** out_ctx);
void lbf_ctx_destroy(lbf_ctx* ctx);
int lbf_ctx_num_devices(const lbf_ctx* ctx);
/* Host-path workers: one per selected device (LBF_WORKERS_PER_DEVICE=k, a
 * test knob read at creation, gives k per device).  A batch is split into
 * contiguous index ranges, one per worker, each on its own host thread. */
int lbf_ctx_num_workers(const lbf_ctx* ctx);
/* Placement of worker `worker` (diagnostics): its device, that device's NUMA
 * node (-1 unknown or LBF_NUMA=0), the NUMA node holding its pinned staging
 * (-1 unknown), and how many CPUs its host threads are bound to (0 unbound).
 * Any output pointer may be NULL. */
int lbf_ctx_worker_info(const lbf_ctx* ctx, int worker, int* device, int* numa_node, int* staging_node,
                        int* bound_cpus);

/* ---- batched chunk hashing (Encoder::EncodeFile's per-chunk hash) --------
 * Chunk i is the byte range [offsets[i], offsets[i] + sizes[i]) of `base`.
 * LBF_HOST_PTR: base/offsets/sizes/out are host memory; `base_len` bounds
 *   the readable range of `base`.  Chunks are streamed through pinned staging
 *   to the context's devices (contiguous index ranges per device).
 * LBF_DEVICE_PTR: everything is device memory of the context's first device
 *   and the call is synchronous on the context stream. */
int lbf_sha1_batch(lbf_ctx* ctx, const uint8_t* base, uint64_t base_len,
                   const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                   uint8_t* out_digests, int flags);

/* ---- batched verify (Flood.cpp:259-275, ChunkMethods.cpp:116-123,165-167)
 * verdicts[i] = 1 when SHA-1(chunk i) equals expected[20*i .. 20*i+20),
 * else 0.  The comparison happens on the device. */
int lbf_verify_batch(lbf_ctx* ctx, const uint8_t* base, uint64_t base_len,
                     const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                     const uint8_t* expected, uint8_t* verdicts, int flags);

/* ---- caller-pinned sources ------------------------------------------------
 * Register [ptr, ptr + len) of caller host memory with the context (pinned
 * for all of its devices; whole pages).  A LBF_HOST_PTR batch whose
 * [base, base + base_len) lies in a registered range is copied to the device
 * straight from it, one H2D per run of adjacent chunks, instead of passing
 * through the context's pinned staging: host DRAM then carries each byte
 * once, not three times (the staging memcpy's read and write, then the DMA
 * read).  Groups of small scattered chunks (runs under 1 MiB on average)
 * still go through staging.  On one MI355X the direct route ran 14 against
 * 12 GiB/s at 64 MiB and 50 against 34-50 GiB/s at 4 GiB.
 * Meant for buffers reused across calls (a peer's receive arenas, a resident
 * file image): the first registration of pages costs about as much as one
 * staged pass over them -- 4 GiB of touched 4 KiB pages 168-233 ms (what new[]
 * and malloc give), 7.5 ms on transparent huge pages, ~700 ms on pages never
 * touched (the registration faults them in) -- and that cost lands in this
 * call, not in the first direct copy; registering pages HIP registered before
 * in the process is cheap, unregistering ~0.03 ms (tools/register_cost.py,
 * profiles/r06/register_cost/).  A call that overlaps pages a running job
 * pinned on the fly (LBF_AUTOPIN=1) waits for
 * that job to end, then pins the range itself.  Memory
 * that is already pinned is accepted and left pinned.  Pinning is per page:
 * ranges held by one context may not share a page (give each registered
 * buffer pages of its own).  Unregister (with the pointer passed here) before
 * freeing the memory; lbf_ctx_destroy unregisters what is left. */
int lbf_host_register(lbf_ctx* ctx, const void* ptr, uint64_t len);
int lbf_host_unregister(lbf_ctx* ctx, const void* ptr);
/* Cumulative chunk bytes this context's host-pointer and file batches sent
 * through its pinned staging and straight from registered memory
 * (diagnostics; either pointer may be NULL). */
int lbf_ctx_staging_stats(lbf_ctx* ctx, uint64_t* staged_bytes, uint64_t* direct_bytes);

/* ---- chunks read straight from a file ------------------------------------
 * Chunk i = bytes [offsets[i], offsets[i] + sizes[i]) of the file at `path`,
 * read with pread into the context's pinned staging (no intermediate copy),
 * overlapped with H2D copies and kernels.  This is EncodeFile's fread loop
 * (Encoder.cpp:54-72) and _SetupFilesAndChunks' fseek/fread loop
 * (Flood.cpp:259-275) batched.
 * expected == NULL: hash mode, `out` receives n*20 digest bytes; a chunk that
 *   cannot be read in full fails the call with LBF_ERR_IO.
 * expected != NULL: verify mode, `out` receives n verdict bytes; a chunk that
 *   cannot be read in full (missing file, past EOF) gets verdict 0, as the
 *   reference leaves such chunks '0'. */
int lbf_file_ranges(lbf_ctx* ctx, const char* path, const uint64_t* offsets, const uint32_t* sizes,
                    uint64_t n, const uint8_t* expected, uint8_t* out);
/* The same over several files in ONE pipelined batch: chunk i is bytes
 * [offsets[i], offsets[i] + sizes[i]) of paths[file_of[i]] (file_of may be
 * NULL when n_files == 1).  This is EncodeFile's loop over m_files
 * (Encoder.cpp:40-79) and _SetupFilesAndChunks' loop over the flood's files
 * (Flood.cpp:239-287) as one call: every chunk's serial SHA-1 chain costs the
 * same whatever the batch, so per-file calls pay it once per file.  Per-chunk
 * semantics as lbf_file_ranges; a file that cannot be opened fails hash mode
 * with LBF_ERR_IO and gives verdict 0 to all its chunks in verify mode. */
int lbf_files_ranges(lbf_ctx* ctx, const char* const* paths, uint32_t n_files, const uint32_t* file_of,
                     const uint64_t* offsets, const uint32_t* sizes, uint64_t n, const uint8_t* expected,
                     uint8_t* out);

/* ---- received chunks as base64 text (ChunkMethods.cpp:137-167) -----------
 * The receiver's two per-chunk passes on the device: XML-RPC's base64 decode
 * of the SendChunk payload (XmlRpcValue.cpp:417-436, xmlrpc++ 0.7
 * base64.h:215-330) and the verify.  Chunk i arrived as the base64 text
 * text[text_offsets[i], + text_lens[i]) (host memory; the bytes between
 * `<base64>` and `</base64>`).  It is decoded with xmlrpc++'s rules --
 * characters outside the alphabet are skipped; the first group of four that
 * holds '=' ends the data ("xx==" one byte, "xxx=" two); an incomplete last
 * group is dropped -- and verdicts[i] = 1 when the decoded length equals
 * expected_sizes[i] (ChunkMethods.cpp:156) and its SHA-1 equals
 * expected[20*i .. 20*i+20).  out_sizes[i] (may be NULL) receives the decoded
 * length, or expected_sizes[i] + 1 when the text decodes to more.  With `out`
 * non-NULL the decoded bytes land at out[out_offsets[i], + expected_sizes[i])
 * (host memory); the bytes of a slot past its decoded length are zeroed,
 * and no byte of `out` outside the slots is written.  Overlapping slots are
 * refused (LBF_ERR_INVALID).  Synchronous, on the context's first device.
 * Text and output in memory registered with lbf_host_register move by DMA
 * without staging.  lbf_ctx_b64_stats counts the chunks whose text had the
 * encoder's own layout (decoded in one pass) and the others.  Of the others,
 * a chunk of more than 54 bytes whose text is its unbroken RFC 4648 text --
 * text_lens[i] == 4 * ceil(expected_sizes[i] / 3) and not
 * lbf_b64_put_length(expected_sizes[i]); what bitflood's Java and Perl peers
 * send -- goes through the flat pass (one pass, no separator places;
 * lbf_set_b64_flat, lbf_ctx_b64_flat_stats) and skips the encoder-layout
 * attempt; the rest, and a candidate that holds anything but alphabet
 * characters and a last group "xx==" / "xxx=", are decoded by the general
 * two-pass kernel.  A chunk of more than 1 GiB (expected_sizes) or
 * 1.5 GiB of text is refused (LBF_ERR_INVALID): the kernels keep positions
 * within a chunk in 32 bits. */
int lbf_b64_verify_batch(lbf_ctx* ctx, const char* text, uint64_t text_len, const uint64_t* text_offsets,
                         const uint32_t* text_lens, uint64_t n, const uint32_t* expected_sizes,
                         const uint8_t* expected, uint8_t* out, uint64_t out_len, const uint64_t* out_offsets,
                         uint32_t* out_sizes, uint8_t* verdicts);

/* ---- chunks to send, encoded as base64 text (ChunkMethods.cpp:89-135) ----
 * The sender's per-chunk passes on the device: the seeder's re-verify
 * (ChunkMethods.cpp:116-123) and XML-RPC's base64 encode of the SendChunk
 * payload (XmlRpcValue::binaryToXml, xmlrpc++ 0.7 base64.h:154-210), from one
 * device copy of the bytes.  Chunk i = data[offsets[i], + sizes[i]) (host
 * memory): verdicts[i] = 1 when its SHA-1 equals expected[20*i .. 20*i+20);
 * its text -- four characters per three bytes, a space (the frame's newline)
 * after every 18th complete group, "xx==" / "xxx=" for a last one or two
 * bytes -- lands at text[text_offsets[i], + lbf_b64_put_length(sizes[i]))
 * whatever the verdict; no byte of `text` outside the slots is written, and
 * overlapping slots are refused (LBF_ERR_INVALID), and so is a chunk of more
 * than 1 GiB.  Synchronous, on the context's first device. */
int lbf_verify_encode_b64_batch(lbf_ctx* ctx, const uint8_t* data, uint64_t data_len, const uint64_t* offsets,
                                const uint32_t* sizes, uint64_t n, const uint8_t* expected, uint8_t* verdicts,
                                char* text, uint64_t text_len, const uint64_t* text_offsets);
/* Chunks of lbf_b64_verify_batch calls on this context so far, by decode
 * path (diagnostics; either pointer may be NULL).  general_chunks reads "not
 * the encoder's layout": it counts the flat pass's candidates too, whichever
 * kernel decoded them (lbf_ctx_b64_flat_stats has their share). */
int lbf_ctx_b64_stats(lbf_ctx* ctx, uint64_t* one_pass_chunks, uint64_t* general_chunks);
/* Length of that text for a chunk of `size` bytes (xmlrpc++'s encoder). */
uint64_t lbf_b64_put_length(uint64_t size);

/* ---- single buffer (Encoder::Base64Encode's hash, host memory) ---------- */
int lbf_sha1_one(lbf_ctx* ctx, const uint8_t* data, uint32_t size, uint8_t out_digest[20]);

/* ---- digest <-> 27-char string (basecode.cpp:39-104, Encoder.cpp:104-105)
 * lbf_b64_27 writes 27 chars + NUL.  lbf_b64_27_decode accepts exactly 27
 * chars of the standard alphabet whose last char carries 4 data bits and 2
 * zero bits; anything else returns LBF_ERR_INVALID. */
void lbf_b64_27(const uint8_t digest[20], char out[28]);
int lbf_b64_27_decode(const char* in, size_t len, uint8_t out_digest[20]);

/* ---- device-resident asynchronous entry points ---------------------------
 * All pointers are device memory on the current HIP device; `stream` is a
 * hipStream_t (NULL = the default stream).  These enqueue and return; they
 * are what bench.py times and what the pipelined host paths use.
 * d_expected/d_verdicts may be NULL (hash only); d_digests may be NULL when
 * only verdicts are wanted. */
int lbf_sha1_launch(const uint8_t* d_base, const uint64_t* d_offsets,
                    const uint32_t* d_sizes, uint64_t n, uint8_t* d_digests,
                    const uint8_t* d_expected, uint8_t* d_verdicts, void* stream);
/* Uniform chunking of one region (one file laid out contiguously):
 * chunk i = [i*chunk_size, min((i+1)*chunk_size, len)), i in [first, first+n). */
int lbf_sha1_uniform_launch(const uint8_t* d_base, uint64_t len, uint32_t chunk_size,
                            uint64_t first_chunk, uint64_t n, uint8_t* d_digests,
                            const uint8_t* d_expected, uint8_t* d_verdicts, void* stream);
/* Kernel variant selection for the two launchers above (0 = automatic):
 * shipped are 1 lane, 7 pc4 (schedule read as 8-byte pairs), 10 pcx5,
 * 11 lds2 and 12 pc4x2; the superseded and diagnostic variants exist only in
 * the A/B library of tools/experimental/, and the shipped library rejects
 * them with LBF_ERR_INVALID.  Exposed for benchmarking and tests; see
 * DESIGN.md "kernels".  lbf_kernel_for(n) is the variant a launch of n
 * chunks runs under the current setting. */
int lbf_set_kernel_variant(int variant);
int lbf_get_kernel_variant(void);
int lbf_kernel_for(uint64_t n_chunks);

/* ---- resumable SHA-1: a chunk hashed piece by piece ------------------------
 * The reference's hash object takes Update() calls of any length and then
 * Final(), which restarts it (Crypto++ 5.2.1 IteratedHash, iterhash.cpp:9-99,
 * iterhash.h:120).  A lbf_sha1_state is that object as a plain record: 96
 * bytes, owned by the caller, copyable (a peer may store it and resume in
 * another context or process).  Invariant: buffered == total % 64.
 * lbf_sha1_state_init is host code and needs no GPU. */
typedef struct lbf_sha1_state {
  uint32_t h[5];      /* chaining value, native words (sha.cpp:19-26 at start) */
  uint32_t buffered;  /* 0..63 bytes of an unfinished block held in `block`    */
  uint64_t total;     /* bytes absorbed so far, the buffered ones included     */
  uint8_t  block[64]; /* the first `buffered` bytes are meaningful             */
} lbf_sha1_state;
void lbf_sha1_state_init(lbf_sha1_state* states, uint64_t n);

/* Device-resident and asynchronous on `stream`, like lbf_sha1_launch: piece i
 * = d_base[d_offsets[i], + d_sizes[i]) is absorbed into state d_state_of[i]
 * (state i when d_state_of is NULL) of d_states[0, n_states), which must be
 * 16-byte aligned.  A piece with d_final[i] != 0 ends its chain: the digest
 * goes to d_digests + 20*i and/or the verdict against d_expected + 20*i to
 * d_verdicts[i], and the state is put back to its initial value.  d_final may
 * be NULL (no piece is final; then no output is needed); d_digests or
 * d_expected/d_verdicts (which go together) may be NULL.  Digest and verdict
 * entries of pieces that are not final are left untouched.  A piece whose
 * state index is >= n_states is skipped (nothing is read or written for it),
 * and `buffered` is taken & 63, so a corrupt record can never make the kernel
 * write outside its own 96 bytes.  Two pieces naming ONE state in one launch
 * is undefined here: memory-safe, but the order they are absorbed in is not
 * defined (feed a chain's pieces in successive launches, or in one launch of
 * lbf_sha1_update_seq_launch below; the batch call refuses it).  The arrays are checked against their allocations
 * as in lbf_sha1_launch. */
int lbf_sha1_update_launch(lbf_sha1_state* d_states, uint64_t n_states, const uint32_t* d_state_of,
                           const uint8_t* d_base, const uint64_t* d_offsets, const uint32_t* d_sizes,
                           const uint8_t* d_final, uint64_t n, uint8_t* d_digests,
                           const uint8_t* d_expected, uint8_t* d_verdicts, void* stream);
/* The same over host memory, synchronous on the context's first device: the
 * touched states and the pieces' bytes (only those, one copy per run of
 * adjacent pieces) go to the device, one launch absorbs them, states and
 * results come back.  out_digests / verdicts entries of pieces that are not
 * final are left untouched.  Checked before any GPU work, each refused with
 * LBF_ERR_INVALID and a message naming the piece, states and outputs
 * untouched: a piece outside [base, base + base_len); state_of[i] >= n_states;
 * two pieces of one state; a state with buffered > 63 or buffered != total %
 * 64; total + size past 2^61 bytes (the bit count is a 64-bit number).
 * Device memory per call is bounded: at most LBF_UPDATE_MB MiB of piece bytes
 * (default 256, read at context creation) go per launch, a larger call runs
 * as successive launches, and a single piece larger than that is cut at
 * multiples of 64 bytes and fed over successive launches.  States and results
 * are written back launch by launch: a HIP failure part-way through such a
 * call leaves the pieces of the launches before it absorbed. */
int lbf_sha1_update_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                          const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                          const uint32_t* sizes, const uint8_t* final_flags, uint64_t n,
                          uint8_t* out_digests, const uint8_t* expected, uint8_t* verdicts);

/* Several pieces of one chain in one launch, absorbed in order.  The pieces are
 * described per piece exactly as for lbf_sha1_update_launch (offsets, sizes,
 * final flags; outputs indexed by piece); which pieces belong to which chain is
 * said by a chain table, CSR style, in place of d_state_of: chain c continues
 * state d_chain_state[c] (state c when d_chain_state is NULL) and its pieces
 * are the piece indices [d_chain_first[c], d_chain_first[c + 1]), absorbed in
 * index order (d_chain_first has n_chains + 1 entries).  One lane per chain
 * holds the record's header in registers from the chain's first piece to its
 * last and writes it once.  A final piece that is not its chain's last piece
 * in the launch is defined HERE (the host call below refuses it): it ends the
 * chunk and writes its outputs, and the pieces behind it begin a new chunk
 * from the initial value -- what successive launches give.  Against a forged
 * table: both ends of a chain's range are clamped to n and an inverted range
 * is empty; a chain whose state index is >= n_states is skipped whole, nothing
 * read or written for it; pieces that no chain names are left alone; a chain
 * of no pieces leaves its record as it is.  Two chains naming ONE state, or
 * one piece named by two chains, stay undefined but memory-safe.  Device-
 * resident and asynchronous on `stream`, one enqueue; the arrays are checked
 * against their allocations as in lbf_sha1_update_launch. */
int lbf_sha1_update_seq_launch(lbf_sha1_state* d_states, uint64_t n_states, const uint32_t* d_chain_state,
                               const uint32_t* d_chain_first, uint64_t n_chains, const uint8_t* d_base,
                               const uint64_t* d_offsets, const uint32_t* d_sizes, const uint8_t* d_final,
                               uint64_t n, uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                               void* stream);
/* lbf_sha1_update_batch without "two pieces of one state": pieces of one state
 * are absorbed in the order they stand in the call, and results come back at
 * the caller's piece indices.  Per launch each touched state travels once,
 * whatever the number of its pieces.  Checked before any GPU work, each refused
 * with LBF_ERR_INVALID and a message naming the piece, states and outputs
 * untouched: everything lbf_sha1_update_batch refuses but that; a state's total
 * plus the SUM of its pieces' sizes past 2^61 bytes; a final piece that is
 * followed by another piece of its state in the same call (feed the next
 * chunk's pieces in the next call).  A call in which no state repeats returns
 * exactly what lbf_sha1_update_batch returns.  Launches are cut by
 * LBF_UPDATE_MB in caller order as there, so a chain's pieces may straddle
 * launches, which are ordered. */
int lbf_sha1_update_seq_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                              const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                              const uint32_t* sizes, const uint8_t* final_flags, uint64_t n,
                              uint8_t* out_digests, const uint8_t* expected, uint8_t* verdicts);

/* ---- resumable base64 decode chained to the resumable SHA-1 ----------------
 * A SendChunk payload is base64 text (ChunkMethods.cpp:137-167) and reaches a
 * receiver in pieces, as the socket delivers them.  A lbf_b64_state is
 * xmlrpc++ 0.7's decoder (base64.h:215-330) stopped between two pieces: 16
 * bytes, owned by the caller, copyable, kept beside the chain's lbf_sha1_state
 * at the same index of a parallel array.  The rule, for pieces: characters
 * outside the alphabet are skipped; the carried sextets and the piece's
 * alphabet characters are taken four at a time; the first '=' ends the data
 * (one more byte with 2 sextets pending, two with 3, none with 0 or 1) and sets
 * `ended`, after which text is ignored; an unfinished group is carried, and on
 * the final piece dropped.  However a text is cut into pieces, the bytes are
 * those of the whole text's decode.  Invariants (the batch call checks them):
 * ncarry <= 3, carry < 2^(6*ncarry), ended <= 1, zero == 0, ended == 0 implies
 * decoded % 3 == 0, decoded < 2^61, and the partner SHA state's total ==
 * min(decoded, chunk size).  lbf_b64_state_init is host code and needs no GPU. */
typedef struct lbf_b64_state {
  uint64_t decoded;  /* bytes the chain's text has decoded to so far (true count, past the slot too) */
  uint32_t carry;    /* the sextets of the unfinished group: sextet k at bits [6k, 6k+6) */
  uint8_t  ncarry;   /* 0..3 */
  uint8_t  ended;    /* 1 once a group holding '=' has ended the data; later text is ignored */
  uint16_t zero;
} lbf_b64_state;
void lbf_b64_state_init(lbf_b64_state* states, uint64_t n);

/* Device-resident and asynchronous on `stream`: four enqueues (three with the
 * line path off, lbf_set_b64_lines) and one more with the flat path on
 * (lbf_set_b64_flat) -- or three in all on the fused route (lbf_set_b64_fused,
 * below: one decode kernel in place of up to three) -- no host round trip, no
 * device allocation.  Piece i = the text d_text[d_text_offsets[i], + d_text_lens[i])
 * continues chain d_state_of[i] (chain i when d_state_of is NULL): the pair
 * d_b64_states[s], d_sha_states[s] of n_states pairs (both arrays 16-byte
 * aligned).  Its chunk's slot is d_out[d_out_offsets[i], + d_caps[i]) -- the
 * caller repeats slot start and chunk size for every piece of a chain -- and
 * the bytes the piece decodes land in it at their position in the chunk; no
 * byte at or past d_caps[i] is written, and no byte of the slot other than the
 * ones the call decodes: what lies below the chain's position and what has not
 * arrived stay as they are, so slots may be packed next to one another.  The
 * line path goes first (one workgroup per piece): the prefix of a piece that
 * continues xmlrpc++'s layout from where the record stands -- groups of four
 * alphabet characters, a separator after every 18th -- is decoded from its
 * known places through tiles of whole lines, each tile validated before it is
 * stored; the record moves on in place and the work arrays carry the count to
 * the next kernel.  The flat path, when switched on, follows (one workgroup
 * per piece; with the line path off it goes first): of what is left it takes
 * the prefix that is unbroken text -- the carried group completed, then whole
 * groups of alphabet characters up to one that holds '=' -- through tiles of
 * 5,184 characters, validated and handed on in the same way.  The last decode
 * kernel takes the rest of every piece by the general rule (one workgroup per
 * piece) and fills the work arrays d_piece_offsets / d_piece_sizes (n entries
 * each, the caller's) with where each piece's new bytes lie;
 * lbf_sha1_update_launch absorbs exactly those; a last kernel clears the
 * verdict of a final piece whose decoded length is not d_caps[i].  A piece
 * with d_final[i] != 0 ends its chain: an unfinished group is dropped,
 * d_out_sizes[i] = the decoded length (d_caps[i] + 1 when more), digest and/or
 * verdict as lbf_sha1_update_launch writes them, and both records are put back
 * to their initial values.  Entries of pieces that are not final are left
 * untouched.  d_out_sizes is required; d_final, d_digests and d_expected /
 * d_verdicts may be NULL as for lbf_sha1_update_launch.  A piece whose state
 * index is >= n_states is skipped, nothing read or written for it; one whose
 * d_caps[i] exceeds 1 GiB decodes nothing, hands the hash an empty piece and
 * gets verdict 0 and d_out_sizes[i] = 0, and when it is final both records are
 * put back all the same.  A forged record (ncarry is taken & 3, carry masked,
 * decoded clamped to 2^61, past every slot, so that no position wraps) can
 * never make the kernel write outside its slot and its records, nor name more
 * than the slot holds in the piece table.  Two pieces of one chain in one launch are
 * undefined as for lbf_sha1_update_launch.  Every array is checked against its
 * allocation. */
int lbf_b64_update_launch(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                          const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                          const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                          const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                          uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                          uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, void* stream);
/* The line path of lbf_b64_update_launch / lbf_b64_update_batch, process-wide:
 * 0 switches it off (exactly the three enqueues of the general rule), anything
 * else on.  Returns the previous value.  Until the first launch or call of
 * this function the value is LBF_B64_LINES's (default on; "0" = off).  Both
 * routes give the same bytes, records, lengths and verdicts; the switch exists
 * so that one process can alternate them. */
int lbf_set_b64_lines(int on);
/* Characters of lbf_b64_update_batch calls on this context so far, by decode
 * path (diagnostics; either pointer may be NULL): their sum is the sum of
 * text_lens of every accepted call.  The text of a chain that has ended counts
 * as scan_chars. */
int lbf_ctx_b64_update_stats(lbf_ctx* ctx, uint64_t* line_chars, uint64_t* scan_chars);
/* The flat path of lbf_b64_verify_batch, lbf_b64_update_launch and
 * lbf_b64_update_batch, process-wide, as lbf_set_b64_lines: 0 switches it off
 * (the enqueues and the routing are exactly those without it), anything else
 * on.  Returns the previous value.  Until the first use or call of this
 * function the value is LBF_B64_FLAT's (default off; "1" = on: the extra
 * enqueue costs text in the encoder's layout more than a run's spread, so a
 * receiver with Java or Perl peers switches it on).  Bytes,
 * records, lengths and verdicts are the same either way. */
int lbf_set_b64_flat(int on);
/* The flat path's share of the two counters above (diagnostics; either pointer
 * may be NULL).  flat_chunks: the chunks of lbf_b64_verify_batch calls that the
 * flat pass decoded -- a sub-count of lbf_ctx_b64_stats' general_chunks.
 * flat_chars: the characters of lbf_b64_update_batch calls that the flat kernel
 * took -- a sub-count of lbf_ctx_b64_update_stats' scan_chars, which keeps
 * counting every character the line path did not take. */
int lbf_ctx_b64_flat_stats(lbf_ctx* ctx, uint64_t* flat_chunks, uint64_t* flat_chars);
/* The fused route of lbf_b64_update_launch / lbf_b64_update_batch,
 * process-wide: anything but 0 switches it on, 0 off (the enqueues are exactly
 * those described above).  Returns the previous value.  Until the first launch
 * or call of this function the value is LBF_B64_FUSED's (default off; "1" =
 * on).  On, a launch is three enqueues whatever the other two switches say:
 * one decode kernel (one workgroup per piece) that reads the chain's record
 * once, runs the line path's, the flat path's and the general rule's stages on
 * the piece one after the other with the record in registers, and writes the
 * record and the work arrays once; then lbf_sha1_update_launch and the length
 * check as above.  lbf_set_b64_lines and lbf_set_b64_flat then say which
 * stages run in front of the general rule; which stage takes which characters
 * of a piece is decided on the device from the text, piece by piece, so text
 * in the encoder's layout and unbroken text may share a launch with both on.
 * Bytes, records, lengths, verdicts, the work arrays and the per-path counters
 * (lbf_ctx_b64_update_stats, lbf_ctx_b64_flat_stats) are the same on both
 * routes, to the character. */
int lbf_set_b64_fused(int on);
/* The same over host memory, synchronous on the context's first device.  Piece
 * i = text[text_offsets[i], + text_lens[i]) of chain state_of[i], whose chunk
 * is expected_sizes[i] bytes and lives at out[out_offsets[i], +
 * expected_sizes[i]).  Checked before any GPU work, each refused with
 * LBF_ERR_INVALID and a message naming the piece, states and outputs
 * untouched: text outside [text, text + text_len); a slot outside out; a state
 * index out of range; two pieces of one state; a broken invariant of either
 * record; a chunk over 1 GiB; slots of different states that overlap.  At most
 * LBF_UPDATE_MB MiB of text go to the device per launch (a larger piece is cut
 * and fed over successive launches).  What comes back: only the bytes this
 * call decoded, at out[out_offsets[i] + bytes decoded before ..) -- no other
 * byte of `out` is written, and nothing is zero-filled: the bytes that have
 * not arrived are the caller's -- the states, and for final pieces
 * out_sizes[i] (may be NULL) and verdicts[i] = 1 when the decoded length is
 * expected_sizes[i] and the SHA-1 of those bytes equals expected[20*i ..).
 * expected and verdicts go together and may be NULL. */
int lbf_b64_update_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states, uint64_t n_states,
                         const uint32_t* state_of, const char* text, uint64_t text_len,
                         const uint64_t* text_offsets, const uint32_t* text_lens, const uint8_t* final_flags,
                         uint64_t n, const uint32_t* expected_sizes, const uint8_t* expected, uint8_t* out,
                         uint64_t out_len, const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts);

/* Several pieces of one chain's text in one launch, decoded and absorbed in
 * order: lbf_b64_update_launch's arrays per piece (the caller still repeats
 * slot start and chunk size for every piece of a chain), and the chain table
 * of lbf_sha1_update_seq_launch in place of d_state_of, naming state PAIRS.
 * Three enqueues whatever the piece count and whatever lbf_set_b64_fused says:
 * a decode kernel with one workgroup per chain, which reads the decoder's
 * record once, runs the line path's, the flat path's and the general rule's
 * stages on each piece in turn (lbf_set_b64_lines / lbf_set_b64_flat say which
 * stages run in front of the general rule, as on the fused route) and writes
 * the record once behind the last piece; lbf_sha1_update_seq_launch over the
 * work arrays with the same table; and the length check of final pieces.
 * Bytes, d_out_sizes, verdicts and the work arrays, each at the piece's index,
 * and both records are what the same pieces give when fed one per launch
 * through lbf_b64_update_launch.  A final piece that is not its chain's last
 * is defined here as for lbf_sha1_update_seq_launch: both records restart and
 * the pieces behind it begin a new chunk (the host call below refuses it).
 * That chunk's pieces must name a slot that does not overlap the ended
 * chunk's: the hash runs behind the decode of the whole launch and reads each
 * piece's bytes from its slot.  A
 * piece whose d_caps[i] exceeds 1 GiB is passed over as lbf_b64_update_launch
 * passes it over, and the chain goes on with the next piece.  The forged-table
 * rules are those of lbf_sha1_update_seq_launch; every array is checked
 * against its allocation. */
int lbf_b64_update_seq_launch(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                              const uint32_t* d_chain_state, const uint32_t* d_chain_first, uint64_t n_chains,
                              const char* d_text, const uint64_t* d_text_offsets, const uint32_t* d_text_lens,
                              const uint8_t* d_final, uint64_t n, uint8_t* d_out, const uint64_t* d_out_offsets,
                              const uint32_t* d_caps, uint32_t* d_out_sizes, uint8_t* d_digests,
                              const uint8_t* d_expected, uint8_t* d_verdicts, uint64_t* d_piece_offsets,
                              uint32_t* d_piece_sizes, void* stream);
/* lbf_b64_update_batch without "two pieces of one state": pieces of one state
 * are decoded and absorbed in the order they stand in the call, and results
 * come back at the caller's piece indices.  Per launch a touched state pair
 * travels once and a chain's decoded bytes come back as one range.  Checked
 * before any GPU work, each refused with LBF_ERR_INVALID and a message naming
 * the piece, states and outputs untouched: everything lbf_b64_update_batch
 * refuses but that (the invariants against each pair as it stands at the call;
 * overlap among the slots of different states); pieces of one state that name
 * different slots or chunk sizes; a final piece that is followed by another
 * piece of its state in the same call.  A call in which no state repeats
 * returns exactly what lbf_b64_update_batch returns, and the calls count in
 * lbf_ctx_b64_update_stats / lbf_ctx_b64_flat_stats as its calls do. */
int lbf_b64_update_seq_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states, uint64_t n_states,
                             const uint32_t* state_of, const char* text, uint64_t text_len,
                             const uint64_t* text_offsets, const uint32_t* text_lens, const uint8_t* final_flags,
                             uint64_t n, const uint32_t* expected_sizes, const uint8_t* expected, uint8_t* out,
                             uint64_t out_len, const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts);

/* ---- resumable base64 encode beside the resumable SHA-1 --------------------
 * The seeder's side of the same wire (ChunkMethods.cpp:89-135: re-verify, then
 * base64-encode the payload), for a chunk that is read or held in pieces: the
 * mirror image of lbf_b64_state.  A lbf_b64_enc_state is the encoder stopped
 * between two pieces: 16 bytes, owned by the caller, copyable, kept beside the
 * chain's lbf_sha1_state at the same index of a parallel array.  Two layouts:
 * xmlrpc++'s lines (base64.h:154-210 as the frame sends them: 72 characters and
 * a space) and the unbroken RFC 4648 text bitflood's Java and Perl peers write
 * (XMLEnvelopeProcessor.java:124, RPC/XML.pm:638).  With P(G) the text position
 * of group G -- 4G + G/18 in lines, 4G unbroken -- a piece of s bytes on a chain
 * that has taken t writes the characters [P(t/3), P((t+s)/3)) of the chunk's
 * text and nothing else (in lines, so, the piece that completes a line's 18th
 * group writes the separator behind it); the (t+s) % 3 bytes left over are
 * carried; a final piece also writes the last group ("xx==" / "xxx=") of a
 * chunk whose size is no multiple of 3, and puts the record back to taken = 0,
 * ncarry = 0, carry = 0 with the layout kept.  However a chunk is cut into
 * pieces, its slot ends up holding the whole chunk's text, lbf_b64_text_length
 * characters.  Invariants (the batch call checks them; the launch masks and
 * clamps): ncarry == taken % 3, carry < 2^(8*ncarry), layout <= 1, zero == 0,
 * taken < 2^61, and the partner SHA state's total == taken.  The two functions
 * below are host code and need no GPU. */
#define LBF_B64_LAYOUT_XMLRPC 0   /* 72 characters + one separator (a space) per line */
#define LBF_B64_LAYOUT_FLAT   1   /* unbroken RFC 4648 text */
typedef struct lbf_b64_enc_state {
  uint64_t taken;   /* bytes of the chunk encoded or carried so far */
  uint32_t carry;   /* the bytes of the unfinished group: byte k at bits [8k, 8k+8) */
  uint8_t  ncarry;  /* 0..2 */
  uint8_t  layout;  /* LBF_B64_LAYOUT_* ; survives the reset after a final piece */
  uint16_t zero;
} lbf_b64_enc_state;
/* Any layout but LBF_B64_LAYOUT_FLAT gives LBF_B64_LAYOUT_XMLRPC. */
void lbf_b64_enc_state_init(lbf_b64_enc_state* states, uint64_t n, int layout);
/* Length of a chunk's whole text: lbf_b64_put_length(size) in lines,
 * 4 * ceil(size / 3) unbroken. */
uint64_t lbf_b64_text_length(uint64_t size, int layout);

/* Device-resident and asynchronous on `stream`: three enqueues -- a small
 * kernel that gives the hash its piece sizes (in d_new_lens, which the last
 * kernel then overwrites), lbf_sha1_update_launch unchanged, and the encode
 * kernel, which runs behind the hash and clears an overflowed final piece's
 * verdict itself -- no host round trip, no device allocation.  Piece i =
 * d_base[d_offsets[i], + d_sizes[i]) continues chain d_state_of[i] (chain i
 * when d_state_of is NULL): the pair d_enc_states[s], d_sha_states[s] of
 * n_states pairs (both arrays 16-byte aligned).  Its chunk's text slot is
 * d_text[d_text_offsets[i], + d_text_caps[i]) -- repeated for every piece of
 * the chain -- and the characters the piece produces land in it at their place
 * in the chunk's text; no byte at or past the cap is written, and no byte of
 * the slot other than those characters, so slots may be packed next to one
 * another at any byte phase.  d_new_offsets[i] is where the new characters lie
 * in d_text (d_text_offsets[i] + their position in the chunk's text, clipped
 * to the cap) and d_new_lens[i] how many were written (clipped at the cap): a
 * streaming seeder sends exactly those.  A piece with d_final[i] != 0 ends its
 * chain: d_text_sizes[i] = the chunk's text length, or d_text_caps[i] + 1 when
 * the text does not fit, in which case d_verdicts[i] is cleared; digest and/or
 * verdict as lbf_sha1_update_launch writes them; both records restart (the
 * layout is kept).  Entries of d_text_sizes, d_digests and d_verdicts of pieces
 * that are not final are left untouched.  d_text_sizes is required; d_final,
 * d_digests and d_expected / d_verdicts may be NULL as for
 * lbf_sha1_update_launch.  The layout is read per piece from the record, so
 * both may share a launch.  A piece whose state index is >= n_states is
 * skipped, nothing read or written for it; one whose cap exceeds
 * lbf_b64_text_length(1 GiB, LBF_B64_LAYOUT_XMLRPC) encodes nothing, hands the
 * hash an empty piece, gets d_new_lens[i] = 0 and, when final, verdict 0 and
 * d_text_sizes[i] = 0 with both records restarted.  A forged record (ncarry is
 * taken from `taken` % 3, carry masked to it, layout & 1, taken clamped below
 * 2^61) can never make the kernel write outside its slot, its two records or
 * its table entries.  Two pieces of one chain in one launch are undefined as
 * for lbf_sha1_update_launch.  Every array is checked against its allocation
 * and its element alignment. */
int lbf_b64_encode_update_launch(lbf_b64_enc_state* d_enc_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                 const uint32_t* d_state_of, const uint8_t* d_base, const uint64_t* d_offsets,
                                 const uint32_t* d_sizes, const uint8_t* d_final, uint64_t n, char* d_text,
                                 const uint64_t* d_text_offsets, const uint32_t* d_text_caps,
                                 uint64_t* d_new_offsets, uint32_t* d_new_lens, uint32_t* d_text_sizes,
                                 uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts, void* stream);
/* The same over host memory, synchronous on the context's first device.  Piece
 * i = data[offsets[i], + sizes[i]) of chain state_of[i], whose chunk's text
 * slot is text[text_offsets[i], + text_caps[i]).  Checked before any GPU work,
 * each refused with LBF_ERR_INVALID and a message naming the piece, states and
 * outputs untouched: a piece outside [data, data + data_len); a slot outside
 * [text, text + text_len); a state index out of range; two pieces of one
 * state; a broken invariant of either record; a chunk over 1 GiB (taken +
 * size) or a cap the launch would refuse; slots of different states that
 * overlap.  At most LBF_UPDATE_MB MiB of piece bytes go to the device per
 * launch (a larger piece is cut where lbf_sha1_update_batch cuts it and fed
 * over successive launches).  What comes back: only the characters this call
 * produced, one copy per run of touching ranges -- no other byte of `text` is
 * written -- the states, new_offsets[i] / new_lens[i] (either may be NULL; the
 * offsets are positions in `text`), and for final pieces text_sizes[i] (may be
 * NULL) and verdicts[i].  expected and verdicts go together and may be NULL. */
int lbf_b64_encode_update_batch(lbf_ctx* ctx, lbf_b64_enc_state* enc_states, lbf_sha1_state* sha_states,
                                uint64_t n_states, const uint32_t* state_of, const uint8_t* data, uint64_t data_len,
                                const uint64_t* offsets, const uint32_t* sizes, const uint8_t* final_flags,
                                uint64_t n, const uint8_t* expected, uint8_t* verdicts, char* text,
                                uint64_t text_len, const uint64_t* text_offsets, const uint32_t* text_caps,
                                uint64_t* new_offsets, uint32_t* new_lens, uint32_t* text_sizes);

/* ---- chunks to send, one-shot, in either peer's text layout ---------------
 * lbf_verify_encode_b64_batch with the layout of the text as an argument, one
 * layout per call (a seeder with peers of both kinds makes two calls): chunk
 * i = data[offsets[i], + sizes[i]) (host memory), verdicts[i] = 1 when its
 * SHA-1 equals expected[20*i .. 20*i+20), and its text lands at
 * text[text_offsets[i], + lbf_b64_text_length(sizes[i], layout)) whatever the
 * verdict -- xmlrpc++'s lines for LBF_B64_LAYOUT_XMLRPC, byte for byte what
 * lbf_verify_encode_b64_batch writes; for LBF_B64_LAYOUT_FLAT the unbroken
 * RFC 4648 text bitflood's Java and Perl peers write
 * (XMLEnvelopeProcessor.java:124, RPC/XML.pm:638): 4 * ceil(size / 3)
 * characters, "xx==" / "xxx=" for a last one or two bytes and nothing else.
 * No byte of `text` outside the slots is written.  Refused with
 * LBF_ERR_INVALID: any other layout, a chunk outside [data, data + data_len),
 * a slot outside [text, text + text_len), overlapping slots, a chunk of more
 * than 1 GiB.  Synchronous, on the context's first device. */
int lbf_verify_encode_b64_layout_batch(lbf_ctx* ctx, const uint8_t* data, uint64_t data_len, const uint64_t* offsets,
                                       const uint32_t* sizes, uint64_t n, const uint8_t* expected, uint8_t* verdicts,
                                       int layout, char* text, uint64_t text_len, const uint64_t* text_offsets);
/* The same for chunks resident in device memory, asynchronous on `stream`:
 * lbf_sha1_launch (the usual kernel selection) followed by the layout's encode
 * kernel and one small kernel, no host round trip and no device allocation.
 * Chunk i = d_data[d_offsets[i], + d_sizes[i]); its text lands at
 * d_text[d_text_offsets[i], + lbf_b64_text_length(d_sizes[i], layout)), and no
 * other byte of d_text is written, so slots may be packed next to one another
 * at any byte phase.  d_digests, or d_expected / d_verdicts (which go
 * together), may be NULL; with all three NULL the call only encodes.  The host
 * cannot read d_sizes, so max_size -- the largest chunk of the call, at most
 * 1 GiB -- sizes the grids.  A chunk with d_sizes[i] > max_size is a caller
 * error that stays defined: nothing outside its slot is written, its text is
 * incomplete, and d_verdicts[i] (when given) is cleared; its digest is still
 * its bytes'.  Two slots that overlap are undefined but memory-safe (the batch
 * call refuses them).  Refused with LBF_ERR_INVALID before anything is
 * enqueued: a layout other than the two LBF_B64_LAYOUT_* values, max_size over
 * 1 GiB, a NULL d_data, d_offsets, d_sizes, d_text or d_text_offsets, n over
 * 2^31-1, a table that is not aligned to its element size or does not fit the
 * allocation it points into.  n == 0 returns LBF_OK and enqueues nothing. */
int lbf_verify_encode_b64_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes, uint64_t n,
                                 uint32_t max_size, uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                 int layout, char* d_text, const uint64_t* d_text_offsets, void* stream);

/* ---- received chunk text resident in device memory, one-shot ---------------
 * lbf_b64_verify_batch for text that already lies in device memory,
 * asynchronous on `stream`: only enqueues -- no allocation, no
 * synchronisation, no context, no host round trip.  All pointers are device
 * memory on the current device.  Chunk i's text is d_text[d_text_offsets[i],
 * + d_text_lens[i]), in either peer layout (xmlrpc++'s lines, or the unbroken
 * RFC 4648 text of the Java and Perl peers) or anything else, chunks of all
 * kinds in one call in any order; it is decoded by xmlrpc++'s rule, exactly as
 * lbf_b64_verify_batch decodes it.  The bytes land at d_out[d_out_offsets[i],
 * + d_expected_sizes[i]); the rest of the slot past the decoded length is
 * zeroed, and nothing outside the slots is written.  d_out_sizes[i] = the
 * decoded length, or d_expected_sizes[i] + 1 when the text decodes to more.
 * d_verdicts[i] = 1 only when the decoded length is d_expected_sizes[i] and
 * the SHA-1 of the bytes equals d_expected[20*i ..); d_digests + 20*i receives
 * the SHA-1 of the min(decoded, expected) bytes in the slot.  d_expected and
 * d_verdicts go together and both may be NULL; d_digests may be NULL; with all
 * three NULL nothing is hashed.  d_out, d_out_offsets, d_out_sizes and d_work
 * (lbf_b64_verify_launch_work(n) = 2 * n bytes) are required.
 * The host cannot read the tables, so max_text_len and max_size -- the longest
 * text and the largest expected size of the call, at most 1.5 GiB and 1 GiB --
 * size the grids.  A chunk over either bound is not decoded: its slot is
 * untouched, d_out_sizes[i] = UINT32_MAX, its verdict is 0 (its digest is the
 * empty string's).  The route is decided per chunk on the device from its own
 * lengths and does not depend on lbf_set_b64_flat: a chunk of more than 54
 * bytes whose text length is 4 * ceil(size / 3) and not lbf_b64_put_length(size)
 * takes the flat tiles, any other the encoder-layout tiles, and a text either
 * cannot take goes to a general scan.  d_work is zeroed first and then holds
 * two arrays a caller (or a test) may read behind the call: d_work[0, n) is
 * `over` (1 = the text decodes to more than the slot), d_work[n, 2n) is `redo`
 * (1 = the chunk went to the general scan).
 * What the launch cannot check for itself is the caller's responsibility: slots
 * that overlap one another, and text that overlaps the output (undefined, but
 * nothing outside the slots and the tables is written); and calls on different
 * streams need different d_work (and different outputs).
 * Refused with LBF_ERR_INVALID before anything is enqueued: a NULL required
 * argument, n over 2^31-1, max_size over 1 GiB or max_text_len over 1.5 GiB,
 * d_expected without d_verdicts or the reverse, digest or expected arrays that
 * are not 4-byte aligned, a table that is not aligned to its element size or
 * does not fit the allocation it points into.  n == 0 returns LBF_OK whatever
 * else is passed and enqueues nothing. */
uint64_t lbf_b64_verify_launch_work(uint64_t n);   /* bytes of d_work: 2 * n */
int lbf_b64_verify_launch(const char* d_text, const uint64_t* d_text_offsets, const uint32_t* d_text_lens,
                          uint64_t n, uint32_t max_text_len,
                          const uint32_t* d_expected_sizes, uint32_t max_size,
                          uint8_t* d_out, const uint64_t* d_out_offsets, uint32_t* d_out_sizes,
                          uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                          uint8_t* d_work, void* stream);

/* ---- the flood file's hash strings on the device ---------------------------
 * bitflood names a chunk by the 27 characters lbf_b64_27 gives for its SHA-1.
 * These two launches keep that form on the device for chunks resident in
 * device memory: Encoder::EncodeFile's strings out, and the resume / seed
 * verify of Flood::_SetupFilesAndChunks (Flood.cpp:259-285) -- string compare,
 * chunkmap, chunks to download -- with no host step before or behind the hash.
 * All pointers are device memory on the current device.  Both calls only
 * enqueue on `stream`: no allocation, no synchronisation, no context, no host
 * read of any table.  Chunk i = d_data[d_offsets[i], + d_sizes[i]), hashed by
 * lbf_sha1_launch itself (the usual kernel selection, lbf_set_kernel_variant
 * included; a chunk of size 0 hashes as the empty string) into d_digests, or
 * into d_work when d_digests is NULL.  d_work is
 * lbf_verify_hashes_launch_work(n) bytes for both calls, 4-byte aligned:
 *   ((20 * n + 15) & ~15) + 4 * ceil(n / 1024)
 * -- the digests, then from the next multiple of 16 one uint32 per 1,024
 * chunks (the count of '0' of that group, then its base in the list).  Calls
 * on different streams need different d_work.
 *
 * lbf_sha1_hashes_launch: string i, 27 characters and no NUL, is written at
 * d_hashes[d_hash_offsets[i], + 27), or at 27 * i when d_hash_offsets is NULL.
 * No other byte of d_hashes is written, so a slot may sit at any byte phase,
 * inside a preformatted hash="..." attribute for example.
 *
 * lbf_verify_hashes_launch: hash i is d_hashes[d_hash_offsets[i],
 * + d_hash_lens[i]); both tables may be NULL together, which means packed
 * 27-byte strings.  d_chunkmap[i] = '1' exactly when d_hash_lens[i] == 27 and
 * the 27 bytes equal the string of chunk i's SHA-1, and '0' in every other
 * case: any other length (0 included), a byte outside the alphabet, a last
 * character with non-zero low bits, another chunk's hash.  The characters are
 * compared, not decoded digests, as chunk.m_hash.compare(test) == 0 does.
 * d_missing and d_missing_count go together and may both be NULL; otherwise
 * d_missing[0, *d_missing_count) holds the indices with '0' in ascending order
 * (d_missing has room for n entries; those past the count are untouched), and
 * *d_missing_count is written by every call with n > 0, also when it is 0.
 * A flood of several files passes its chunks in the flood's order (map order
 * of the file names, then chunk index): each file's chunkmap is then a
 * contiguous slice of d_chunkmap, and the caller maps the list's entries back
 * to (name, index).
 *
 * Refused with LBF_ERR_INVALID before anything is enqueued: a NULL d_data,
 * d_offsets, d_sizes, d_hashes, d_work or (verify) d_chunkmap, n over 2^31-1,
 * d_hash_offsets without d_hash_lens or d_missing without d_missing_count or
 * the reverse, d_digests or d_work not 4-byte aligned, a table that is not
 * aligned to its element size or does not fit the allocation it points into
 * (strings addressed through d_hash_offsets are the caller's to place).
 * n == 0 returns LBF_OK, enqueues nothing and writes nothing,
 * *d_missing_count included. */
int lbf_sha1_hashes_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes, uint64_t n,
                           char* d_hashes, const uint64_t* d_hash_offsets /* NULL: 27 * i */,
                           uint8_t* d_digests /* may be NULL */, uint8_t* d_work, void* stream);
uint64_t lbf_verify_hashes_launch_work(uint64_t n);   /* bytes of d_work, for both calls */
int lbf_verify_hashes_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes, uint64_t n,
                             const char* d_hashes, const uint64_t* d_hash_offsets, const uint32_t* d_hash_lens,
                             char* d_chunkmap, uint32_t* d_missing, uint32_t* d_missing_count,
                             uint8_t* d_digests /* may be NULL */, uint8_t* d_work, void* stream);

/* ---- a receive stream on the device: frames, SendChunk frames, chunks ------
 * lbf_b64_verify_launch takes tables in device memory that name each chunk's
 * text, size and hash.  These two launches fill them from the raw bytes a
 * receiver holds in device memory, so that stream -> bytes and verdicts needs
 * no host read in between: the '\n' frame split of the peer loop, and
 * PeerWire::LocateSendChunk on every frame, which is the specification of the
 * second call -- kind, index, text range and name range agree with it on every
 * frame, well-formed or not.  All pointers are device memory on the current
 * device.  Both calls only enqueue on `stream`: no allocation, no
 * synchronisation, no context, no host read of any table.  Calls on different
 * streams need different d_work.
 *
 * lbf_wire_frames_launch splits d_stream[0, stream_len) on '\n'.  Frame k is
 * the bytes between delimiter k-1 and delimiter k, without the delimiter; an
 * empty frame is a frame of length 0.  The first min(found, max_frames) frames
 * are written in stream order to d_frame_offsets / d_frame_lens (entries past
 * that are untouched), *d_n_frames is the number found, also when it exceeds
 * max_frames, and *d_tail is the offset of the first byte behind the last
 * delimiter (0 when there is none, stream_len when the stream ends in one):
 * the unfinished frame the receiver carries into its next pass.  max_frames ==
 * 0 with both tables NULL counts only.  The stream may start and end at any
 * byte phase; no byte outside it is read for its value.  d_work is
 * lbf_wire_frames_launch_work(stream_len) bytes, 4-byte aligned:
 *   4 * ceil((stream_len + 15) / 4096)
 * -- one uint32 per 4,096 bytes, counted from the aligned 16-byte block that
 * holds the stream's first byte.  Refused with LBF_ERR_INVALID before anything
 * is enqueued: a NULL d_stream, d_n_frames, d_tail or d_work, stream_len over
 * 2^32-1 (a larger arena is passed as windows), one of d_frame_offsets,
 * d_frame_lens and max_frames without the others, a table that is not aligned
 * to its element size or does not fit the allocation it points into.
 * stream_len == 0 returns LBF_OK, enqueues nothing and writes nothing.
 *
 * lbf_wire_send_chunks_launch looks at the live frames: the first
 * min(*d_n_frames, n_frames), or n_frames when d_n_frames is NULL.  d_frames[i]
 * is written for each of them (entries past the live count are untouched):
 * LBF_FRAME_OTHER with every other field 0 where LocateSendChunk returns false
 * (or the frame is longer than 1.5 GiB + 64 KiB, or not inside the stream:
 * such a frame is not read); otherwise the ranges as offsets into d_stream,
 * the name as it stands in the frame, still XML-escaped.
 * The flood table (all NULL / 0 together) names the files in the flood's order
 * as lbf_verify_hashes_launch takes them: file f's name, in XmlEncode form, is
 * d_file_names[d_file_name_offsets[f], d_file_name_offsets[f+1]), its chunks
 * are the global numbers [d_file_first[f], d_file_first[f+1]), and chunk c has
 * d_chunk_sizes[c] bytes and the digest d_chunk_expected[20 c, + 20).  A
 * located frame is LBF_FRAME_SEND_CHUNK when its raw name bytes equal a file's
 * entry, its index is below that file's chunk count and the global number is
 * below n_chunks; otherwise LBF_FRAME_SEND_CHUNK_UNBOUND (a name escaped in
 * another way included: that frame is the host's to handle).
 * The dense tables (all NULL / 0 together) receive the bound frames in frame
 * order, entry j < max_chunks: d_text_offsets[j], d_text_lens[j],
 * d_expected_sizes[j], d_expected[20 j, + 20), d_chunk_of[j] (the global chunk
 * number) and d_frame_of[j].  *d_n_located is the number bound, also when it
 * exceeds max_chunks.  Entries [min(located, max_chunks), max_chunks) are made
 * neutral by every call: offset 0, text length 0, expected size 0, an all-zero
 * digest (not SHA-1 of the empty string, so the verdict is 0), d_chunk_of =
 * d_frame_of = UINT32_MAX.  lbf_b64_verify_launch(d_stream, d_text_offsets,
 * d_text_lens, max_chunks, ...) can therefore be enqueued straight behind it,
 * whatever arrived.  Two frames for one chunk both appear.  d_work is
 * lbf_wire_send_chunks_launch_work(n_frames) bytes, 4-byte aligned:
 *   4 * n_frames + 4 * ceil(n_frames / 256)
 * -- a frame's chunk number, then one uint32 per 256 frames.  Refused with
 * LBF_ERR_INVALID before anything is enqueued: half of the flood table or of
 * the dense tables, n_files > 0 with n_chunks == 0, n_frames or max_chunks
 * over 2^31-1, with n_frames > 0 a NULL d_stream, d_frame_offsets,
 * d_frame_lens, d_frames or d_work, a table that is not aligned to its element
 * size or does not fit the allocation it points into (the names addressed
 * through d_file_name_offsets are the caller's to place).  n_frames == 0
 * returns LBF_OK and enqueues nothing, except that dense tables, when given,
 * are made neutral and *d_n_located = 0. */
#define LBF_FRAME_OTHER 0               /* not a well-formed SendChunk frame */
#define LBF_FRAME_SEND_CHUNK 1          /* located and bound to a chunk of the flood table */
#define LBF_FRAME_SEND_CHUNK_UNBOUND 2  /* located; file not in the table, index past the file's
                                           chunks, or no table given */
typedef struct lbf_wire_frame {   /* 32 bytes; offsets are positions in d_stream */
  uint64_t text_offset;  /* first character behind <base64> */
  uint64_t name_offset;  /* the file name as it stands in the frame (still XML-escaped) */
  uint32_t text_len;     /* up to the next '<', exactly what DecodeSendChunk decodes */
  uint32_t name_len;
  uint32_t index;        /* bit for bit LocateSendChunk's o_index */
  uint32_t kind;
} lbf_wire_frame;

uint64_t lbf_wire_frames_launch_work(uint64_t stream_len);
int lbf_wire_frames_launch(const char* d_stream, uint64_t stream_len,
                           uint64_t* d_frame_offsets, uint32_t* d_frame_lens, uint32_t max_frames,
                           uint32_t* d_n_frames, uint64_t* d_tail, uint8_t* d_work, void* stream);

uint64_t lbf_wire_send_chunks_launch_work(uint64_t n_frames);
int lbf_wire_send_chunks_launch(const char* d_stream, uint64_t stream_len,
        const uint64_t* d_frame_offsets, const uint32_t* d_frame_lens, uint32_t n_frames,
        const uint32_t* d_n_frames /* NULL: n_frames is exact */,
        /* flood table, all NULL / 0 together: */
        const char* d_file_names, const uint32_t* d_file_name_offsets /* n_files + 1 */,
        const uint32_t* d_file_first /* n_files + 1 */, uint32_t n_files,
        const uint32_t* d_chunk_sizes, const uint8_t* d_chunk_expected, uint32_t n_chunks,
        lbf_wire_frame* d_frames,
        /* dense tables lbf_b64_verify_launch reads, all NULL / 0 together: */
        uint64_t* d_text_offsets, uint32_t* d_text_lens, uint32_t* d_expected_sizes, uint8_t* d_expected,
        uint32_t* d_chunk_of, uint32_t* d_frame_of, uint32_t max_chunks, uint32_t* d_n_located,
        uint8_t* d_work, void* stream);

/* Synthetic bytes (counter-mode splitmix64): fill
 * d_buf[0..len) with stream `seed` starting at stream byte `start`
 * (start % 8 == 0, d_buf 16-byte aligned). */
int lbf_fill_synthetic(uint8_t* d_buf, uint64_t len, uint64_t seed, uint64_t start, void* stream);

/* Tiny device-memory helpers so C/ctypes callers need no HIP headers. */
int lbf_dev_malloc(void** out_ptr, uint64_t bytes);
int lbf_dev_free(void* ptr);
int lbf_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int lbf_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int lbf_set_device(int device);
int lbf_device_synchronize(void);
int lbf_stream_create(void** out_stream);
int lbf_stream_destroy(void* stream);
int lbf_stream_synchronize(void* stream);
/* Time `reps` back-to-back launches of lbf_sha1_uniform_launch on `stream`
 * with HIP events recorded on that stream; writes the mean ms per launch. */
int lbf_time_uniform(const uint8_t* d_base, uint64_t len, uint32_t chunk_size,
                     uint64_t first_chunk, uint64_t n, uint8_t* d_digests, int reps,
                     void* stream, float* out_ms_per_launch);

#ifdef __cplusplus
}
#endif

#endif /* LBF_HASH_H_ */
