/*
 * mtg_boss.h -- C ABI of the MI355X BOSS chunk constructor (libmtg_boss.so).
 *
 * Drop-in boundary for MetaGraph's in-memory succinct `build` path.  Each entry point replaces
 * one member of the reference's chunk-constructor interface (paths relative to
 * /root/reference/metagraph/src):
 *
 *   mtg_boss_ctor_create        IBOSSChunkConstructor::initialize
 *                               graph/representation/succinct/boss_chunk_construct.hpp:18-34,
 *                               boss_chunk_construct.cpp:1134-1178 (same 9 parameters + device)
 *   mtg_boss_ctor_add_sequences IBOSSChunkConstructor::add_sequences(vector<pair<string,u64>>&&)
 *                               boss_chunk_construct.hpp:26-30 (thread-safe, copies the input)
 *   mtg_boss_ctor_add_sequence  IBOSSChunkConstructor::add_sequence(string_view, u64 count)
 *   mtg_boss_ctor_build_chunk   IBOSSChunkConstructor::build_chunk -> BOSS::Chunk
 *                               (boss_chunk.hpp:19-104: W, last, F, weights, k, alph_size = 5)
 *   mtg_boss_ctor_get_k         IBOSSChunkConstructor::get_k (BOSS k = DBG k - 1)
 *   mtg_boss_chunk_free / mtg_boss_ctor_destroy   the destructors
 *   mtg_last_error              logger->error + exit(1) / throw of the reference become
 *                               negative return codes plus this message
 *
 * Beyond the reference's interface, for callers that already hold reads in HBM (benchmarks,
 * multi-GPU shards): mtg_boss_build_device runs the whole path on a device buffer and leaves
 * the BOSS arrays in device memory; mtg_boss_last_timings reports per-stage device times.
 *
 * Multi-GPU (one process per GPU, RCCL over xGMI): every rank calls the *_dist variant with its
 * own reads and gets the chunk of one range of BOSS order; the rank chunks concatenate in rank
 * order with BOSS::Chunk::extend (boss_chunk.cpp:230-270) into the chunk a single build of all
 * reads returns: one exchange-based build where the reference shards by suffix.
 *
 * The suffix-sharded route itself (`build --suffix-len`, `concatenate --clear-dummy`,
 * cli/build.cpp:102-155, 358-456) runs too: a constructor created with a filter_suffix builds the
 * chunk of that node suffix, and mtg_boss_write_dbg with mask_dummy = 2 prunes the concatenated
 * chunks' redundant source dummies (on the device: mtg_boss_chunk_extend_device, then
 * mtg_boss_write_dbg_device_pruned).
 *
 * No torch types, no C++ types: plain pointers and sizes.  All functions are thread-safe
 * except that one constructor must not be built and added to at the same time.
 */
#ifndef MTG_BOSS_H
#define MTG_BOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTG_BOSS_ABI_VERSION 8

/* container types of the reference (kmer::ContainerType) */
#define MTG_CONTAINER_VECTOR 0
#define MTG_CONTAINER_VECTOR_DISK 1

/* return codes */
#define MTG_OK 0
#define MTG_ERR_INVALID_K -1        /* k not in [1, 84]      (reference: exit(1)) */
#define MTG_ERR_COUNT_WIDTH -2      /* bits_per_count > 32   (reference: runtime_error) */
#define MTG_ERR_UNSUPPORTED -3      /* a multi-GPU build with a filter suffix */
#define MTG_ERR_DEVICE -4           /* HIP runtime / kernel failure */
#define MTG_ERR_ARGUMENT -5
#define MTG_ERR_NO_DEVICE -6        /* no MI355X visible: the product path never falls back */

typedef struct mtg_boss_params {
    uint64_t k;                  /* BOSS k (node length) = DBG k - 1, in [1, 84] */
    int both_strands;            /* canonical mode: add reverse complements */
    uint8_t bits_per_count;      /* 0 = no weights; else --count-width (<= 32) */
    const char *filter_suffix;   /* NULL / "": the full construction; else chars of "$ACGT", shorter
                                    than k + 1: the chunk of the (k+1)-mers whose node ends with it
                                    (boss_chunk_construct.cpp:946-1013); copied at create */
    uint64_t num_threads;        /* host threads for input staging */
    double memory_preallocated;  /* bytes of device memory the build may use (0 = all free HBM);
                                    larger inputs are built in key-range batches */
    int container_type;          /* MTG_CONTAINER_VECTOR, or MTG_CONTAINER_VECTOR_DISK (--disk-swap):
                                    the bounded-memory build, in key-range batches; when even the real
                                    edges would not fit memory_preallocated, build_chunk spills: one
                                    range's edges in HBM at a time, the rest in host memory / swap_dir */
    const char *swap_dir;        /* the disk container's spill files go here (copied at create) */
    uint64_t disk_cap_bytes;     /* at most this many bytes of spill files; further blocks stay in RAM */
    int device_id;               /* HIP device ordinal */
} mtg_boss_params;

typedef struct mtg_boss_ctor mtg_boss_ctor;

/* BOSS::Chunk in host memory (arrays of n entries including the leading row 0).  The arrays are
   pinned host blocks owned by the chunk: release them with mtg_boss_chunk_free. */
typedef struct mtg_boss_chunk {
    uint64_t k;
    uint64_t alph_size;          /* 5: $ACGT */
    uint64_t n;
    uint8_t *W;                  /* n labels 0..9 (int_vector width 4 in the reference) */
    uint64_t *last;              /* n bits, packed: row i is bit i % 64 of word i / 64 (the
                                    sdsl::bit_vector layout of the reference's last_) */
    uint32_t *weights;           /* n weights or NULL (bits_per_count == 0) */
    uint64_t F[5];
    uint8_t bits_per_count;
    uint64_t n_real;             /* real (non-dummy) edges */
    uint64_t n_dummy;            /* dummy edges incl. the main dummy row */
} mtg_boss_chunk;

/* BOSS::Chunk left in device memory (owned by the constructor, valid until its next build) */
typedef struct mtg_boss_device_chunk {
    uint64_t k;
    uint64_t n;
    uint8_t *W;                  /* device pointers */
    uint8_t *last;
    uint32_t *weights;
    uint64_t F[5];
    uint64_t n_real;
    uint64_t n_dummy;
} mtg_boss_device_chunk;

typedef struct mtg_boss_timings {
    double total_ms;             /* device time of the whole path (events on the build stream) */
    double extract_ms;           /* K1 */
    double sort_ms;              /* K2 over the extracted k-mers */
    double unique_ms;            /* K3 */
    double rc_ms;                /* K4 incl. its re-sort */
    double dummy_ms;             /* K5/K6 incl. dummy sort + unique */
    double merge_ms;             /* K7 */
    double emit_ms;              /* K8 */
    double radix_pass_ms;        /* K2's first partition pass (MSD) or average onesweep pass (LSD) */
    double radix_bytes;          /* algorithmic bytes of that launch: 2 n (key + count) */
    uint64_t radix_launches;     /* launches averaged into radix_pass_ms */
    uint64_t n_positions;        /* window starts offered to the extractor */
    uint64_t n_extracted;        /* valid k-mers extracted (N) */
    uint64_t n_unique;           /* distinct k-mers collected (U) */
    uint64_t n_real;             /* real edges after rc augmentation */
    uint64_t n_dummy;            /* dummy edges (sinks + all source levels) */
    uint64_t n_rows;             /* BOSS rows incl. row 0 */
    double exchange_ms;          /* multi-GPU: time inside the exchanges (RCCL) */
    uint64_t n_sent;             /* multi-GPU: elements sent to other ranks */
    uint64_t world;              /* ranks of the build (1 = single GPU) */
    /* host-buffer builds (mtg_boss_ctor_build_chunk): wall times of the host-side stages */
    double stage_ms;             /* add_* calls since the previous build (reads packed to 2-bit codes + a
                                    valid mask in pinned memory, DMA'd to HBM piece by piece meanwhile) */
    double h2d_ms;               /* the wait for the last read pieces + their unpack in HBM */
    double d2h_ms;               /* W, packed last, weights -> pinned host blocks */
    double host_total_ms;        /* the whole build_chunk call */
    uint64_t n_batches;          /* key-range batches of the build (1 = the input fit at once) */
    uint64_t peak_bytes;         /* device workspace held at the end of the build */
    double input_ms;             /* host-buffer builds: KMC decode + FASTA split on the device (incl. their copies) */
    uint64_t spilled_bytes;      /* bytes the build kept outside HBM (the disk container's spill; 0 = none) */
    uint64_t spec_levels;        /* speculative final MSD levels that completed (sample-sized buckets) */
    uint64_t spec_fine_levels;   /* of those, levels sampled per tile (the final level of 3-level plans) */
    uint64_t spec_fallbacks;     /* speculative levels that overflowed and reran as the exact level */
    uint64_t collect_mode;       /* how the real k-mers were collected: 0 one pass, 1 key ranges re-scanning
                                    the reads (both strands), 2 canonical rounds of the fused extraction */
    uint64_t sent_bytes;         /* multi-GPU: bytes this rank sent to the other ranks (every exchange) */
    uint64_t spec_l1;            /* 1: the fused extraction scattered into the speculative level-1 layout
                                    (a sampled histogram pass) */
    uint64_t cached_bytes;       /* device blocks the workspace keeps idle for the next build (counted in
                                    peak_bytes; freed when a build ends without reusing them, or by
                                    mtg_boss_ctor_trim) */
    double exchange_hidden_ms;   /* multi-GPU: exchange time spent while the build stream sorted (the pieces of
                                    exchange 1 in flight under the owner sort of the previous piece) */
    uint64_t coresident;         /* multi-GPU: ranks sharing this rank's GPU (same host name and PCI bus id);
                                    they split its free HBM when planning rounds */
    uint64_t rc_spec_l1;         /* the rc sort's level 1 fused with the rc map: 1 its buckets were sized from a
                                    sample of the canonical set, 2 one of them overflowed and the exact
                                    histogram pass ran instead, 0 neither (not fused, or MTG_RC_SPEC=0).
                                    Appended like the fields before it, with MTG_BOSS_ABI_VERSION unchanged:
                                    mtg_boss_last_timings writes sizeof(mtg_boss_timings) of this header, so a
                                    caller must be compiled against the header of the library it loads */
} mtg_boss_timings;

int mtg_boss_abi_version(void);
const char *mtg_last_error(void);

mtg_boss_ctor *mtg_boss_ctor_create(const mtg_boss_params *params);
void mtg_boss_ctor_destroy(mtg_boss_ctor *ctor);
uint64_t mtg_boss_ctor_get_k(const mtg_boss_ctor *ctor);
/* frees the device memory the constructor holds between builds: the blocks its workspace keeps idle
   (timings' cached_bytes) and the last build's stage buffers; the last build's device chunk arrays
   (W, last, weights) stay valid.  A build also frees, when it ends, the kept blocks it did not reuse */
int mtg_boss_ctor_trim(mtg_boss_ctor *ctor);

/* n sequences, seqs[i] of lens[i] bytes, counts[i] (NULL = all 1).  Copies the input. */
int mtg_boss_ctor_add_sequences(mtg_boss_ctor *ctor, const char *const *seqs,
                                const uint64_t *lens, const uint64_t *counts, size_t n);
int mtg_boss_ctor_add_sequence(mtg_boss_ctor *ctor, const char *seq, uint64_t len,
                               uint64_t count);
/* one packed buffer: n sequences back to back, offsets[n + 1] */
int mtg_boss_ctor_add_packed(mtg_boss_ctor *ctor, const char *data, const uint64_t *offsets,
                             const uint64_t *counts, size_t n);

/*
 * A FASTA or FASTQ file (plain or gzip) as input, the reference's parse_sequences ->
 * read_fasta_file_critical path (cli/parse_sequences.hpp:103-151, seq_io/sequence_io.cpp:364-405)
 * and push_sequences' one-thread-per-file loop (cli/build.cpp:31-56): the calling thread reads and
 * inflates the file into pinned memory; at build time its bytes go to HBM in one copy and are split
 * into records on the device (kseq rules: FASTA header lines start with '>', sequence lines are
 * joined, line ends dropped; FASTQ four-line records).  Each record is one sequence of count 1.
 * Thread-safe; call it concurrently for different files.
 */
int mtg_boss_ctor_add_fasta(mtg_boss_ctor *ctor, const char *path);

/*
 * Contigs with per-k-mer counts as input: the `--count-kmers` branch of parse_sequences
 * (cli/parse_sequences.hpp:103-143) over read_extended_fasta_file_critical
 * (seq_io/sequence_io.cpp:407-467), the pair `metagraph clean` / `transform --to-fasta` write.  Names as
 * in the reference: base = path without a trailing ".gz" and then without ".fasta"; the sequences are
 * base.fasta.gz and the counts base.kmer_counts.gz (a u32 k-mer length, then one u32 per k-mer of every
 * record in file order); either file may be plain or gzip (by its magic bytes).  The reference cuts every
 * record into its runs of equal counts and adds each run with its count; here the calling thread reads
 * and inflates both files into pinned memory, and at build time the records are split on the device and
 * the runs become (start, count) pairs over the unsegmented sequence (csrc/kmer_counts.hpp), staged
 * behind the reads, the KMC records and the plain FASTA files.  Counts above the count width's maximum
 * saturate as those of mtg_boss_ctor_add_sequences do.  Thread-safe; one thread per file.
 * Refused here with MTG_ERR_ARGUMENT, nothing staged: a file that cannot be read, a counts file shorter
 * than 4 bytes, counts for another k than the constructor's k + 1, a payload that is no multiple of 4
 * bytes, FASTQ content, a constructor with bits_per_count == 0 (the reference takes this branch only
 * under --count-kmers: use mtg_boss_ctor_add_fasta).  Refused by build_chunk[_dist] with
 * MTG_ERR_ARGUMENT: a record shorter than k, fewer or more counts than the records have k-mers.
 * A constructor with a filter_suffix returns MTG_ERR_UNSUPPORTED: on that route the reference pads every
 * equal-count segment with '$' as a sequence of its own, which adds dummy edges per segment; that is not
 * built.  Not covered either: the with_reverse flag (both strands' counts are the both_strands build).
 */
int mtg_boss_ctor_add_fasta_counts(mtg_boss_ctor *ctor, const char *path);

/*
 * A KMC1 k-mer counter database (`<base>.kmc_pre` + `<base>.kmc_suf`; either name or the base) as
 * input: seq_io::read_kmers (seq_io/kmc_parser.cpp:27-62) + the build's KMC branch
 * (cli/parse_sequences.hpp:50-101).  Every k-mer with min_count <= count < max_count becomes a
 * one-k-mer sequence with that count; with call_both_from_canonical and a database of canonical
 * k-mers, its reverse complement too (the reference passes graph_mode != CANONICAL).  The
 * records are decoded on the device at build time.  Reference defaults: 1, 2^32 - 1.
 */
int mtg_boss_ctor_add_kmc(mtg_boss_ctor *ctor, const char *kmc_path, uint64_t min_count,
                          uint64_t max_count, int call_both_from_canonical);

/*
 * A KMC1 database decoded straight into device memory, as mtg_boss_ctor_add_kmc decodes it at build
 * time (k bases + '$' per record, its reverse complement after it with call_both_from_canonical on
 * a canonical database), with per-read starts and counts: the input of mtg_boss_build_device[_dist]
 * for a build whose KMC input is already resident in HBM (BASELINE config 5).  Free with
 * mtg_device_reads_free.
 */
typedef struct mtg_device_reads {
    uint8_t *seq;                /* device pointers */
    uint64_t seq_len;
    uint64_t *read_starts;
    uint32_t *counts;
    uint64_t n_reads;            /* records (x2 with reverse complements) */
    int device_id;
} mtg_device_reads;
int mtg_kmc_load_device(const char *kmc_path, uint64_t min_count, uint64_t max_count,
                        int call_both_from_canonical, int device_id, mtg_device_reads *out);
void mtg_device_reads_free(mtg_device_reads *reads);

/*
 * The device step of mtg_boss_ctor_add_fasta_counts alone, for callers that hold everything in HBM: the
 * record starts of a read buffer (record r = [d_record_starts[r], d_record_starts[r + 1] - 1), one
 * separator byte after every record; n_records + 1 entries) and the records' k-mer counts (one per
 * window, record after record: the counts file's payload) -> the runs of equal counts of
 * cli/parse_sequences.hpp:120-138 as `out->read_starts` / `out->counts` / `out->n_reads`, exactly what
 * mtg_boss_build_device takes as d_read_starts / d_counts / n_reads next to the same buffer.  out->seq
 * stays NULL; free `out` with mtg_device_reads_free.  k is the DBG k (BOSS k + 1).  MTG_ERR_ARGUMENT: a
 * record shorter than k ("Bad fasta file. Found sequence shorter than k-mer length"), fewer counts than
 * windows ("Cannot read k-mer features") or more ("There are features left in extension unread").  Takes
 * the constructor's mutex and runs on `stream` (NULL = its own) with its scratch, like the device writers.
 * On return the call has synchronised `stream` (n_reads is a host value), the two arrays are complete, and
 * the constructor's own stream is restored whatever the return code.
 */
int mtg_kmer_counts_to_reads_device(mtg_boss_ctor *ctor, const uint64_t *d_record_starts /* n_records + 1 */,
                                    uint64_t n_records, const uint32_t *d_kmer_counts, uint64_t n_counts,
                                    unsigned k /* DBG k */, void *stream, mtg_device_reads *out);

/*
 * The builder's own k-mer counter: counts the k-mers (k <= 32; canonical = KMC's canonical form,
 * the lexicographically smaller strand) of device-resident reads on the constructor's device and
 * writes them as a KMC1 database <outbase>.kmc_pre / .kmc_suf (record order, prefix table and
 * header as KMC writes them; counts saturate at the counter_size-byte maximum).  Input generator
 * for BASELINE config 5 (the reference takes its KMC databases from KMC itself).  *n_written (may
 * be NULL) = records written.
 */
int mtg_kmc_write_device(mtg_boss_ctor *ctor, const uint8_t *d_seq, uint64_t seq_len, unsigned k,
                         int canonical, unsigned counter_size, unsigned lut_len, const char *outbase,
                         uint64_t *n_written);

/* builds from everything added so far, returns host arrays; clears the added input */
int mtg_boss_ctor_build_chunk(mtg_boss_ctor *ctor, mtg_boss_chunk *out);
void mtg_boss_chunk_free(mtg_boss_chunk *chunk);

/*
 * Device-resident input: `d_seq` holds the reads back to back, each followed by at least one
 * byte outside {A,C,G,T,U,a,c,g,t,u} (so no k-mer spans two reads).  d_read_starts/d_counts
 * (both NULL, or n_reads entries) give per-read counts for --count-kmers.  `stream` is a
 * hipStream_t (NULL = the constructor's own stream).  Arrays stay in device memory.
 * On return the call has synchronised `stream` (n, F and the totals are host values), the arrays are
 * complete, and the constructor's own stream is restored whatever the return code.
 */
int mtg_boss_build_device(mtg_boss_ctor *ctor, const uint8_t *d_seq, uint64_t seq_len,
                          const uint64_t *d_read_starts, const uint32_t *d_counts,
                          uint64_t n_reads, void *stream, mtg_boss_device_chunk *out);

int mtg_boss_last_timings(const mtg_boss_ctor *ctor, mtg_boss_timings *out);

/*
 * Multi-GPU exchange.  mtg_comm_get_unique_id on one rank, broadcast the 128 bytes (e.g. with
 * torch.distributed or MPI), then mtg_comm_create_rccl on every rank with its device.
 * mtg_comm_create_local makes `world` ranks inside one process sharing one device (each rank
 * builds from its own host thread) -- the same exchange semantics without RCCL, for tests.
 */
#define MTG_COMM_ID_BYTES 128
typedef struct mtg_comm mtg_comm;
int mtg_comm_get_unique_id(uint8_t *id /* MTG_COMM_ID_BYTES */);
mtg_comm *mtg_comm_create_rccl(const uint8_t *id, int world, int rank, int device_id);
int mtg_comm_create_local(int world, mtg_comm **comms /* world entries */);
void mtg_comm_destroy(mtg_comm *comm);
int mtg_comm_rank(const mtg_comm *comm);
int mtg_comm_size(const mtg_comm *comm);
/*
 * Local groups created with MTG_LOCAL_SERIAL=1 in the environment hand the device to one rank at a
 * time (from build start to its next exchange, and between exchanges): a step's wall time is then
 * the sum of the ranks' work.  Returns this rank's accumulated device time in ms (reset != 0 zeroes
 * it), -1 for other communicators.  A measurement aid (tools/dist_sim.py), not a build mode.
 */
double mtg_comm_local_held_ms(mtg_comm *comm, int reset);

/*
 * The same exchange over caller-supplied functions on HOST buffers (each returns 0 on success): the
 * library stages every step's device data through host memory and calls them from the building
 * thread.  Any transport carries the build this way (torch.distributed over gloo, MPI, sockets);
 * RCCL over xGMI stays the fast path.  alltoallv: the bytes for rank j are send[sum scnt[0..j)]..
 * (scnt[j] bytes), the bytes from rank i land at recv[sum rcnt[0..i)]...
 */
typedef struct mtg_comm_callbacks {
    void *user;
    int rank;
    int world;
    int (*allreduce_sum_u64)(void *user, uint64_t *buf, size_t n);
    int (*allgather_u64)(void *user, const uint64_t *send, uint64_t *recv, size_t n);
    int (*alltoallv)(void *user, const void *send, const uint64_t *scnt, void *recv, const uint64_t *rcnt);
} mtg_comm_callbacks;
mtg_comm *mtg_comm_create_callbacks(const mtg_comm_callbacks *callbacks);

/* this rank's chunk of the global build (host input staged with mtg_boss_ctor_add_*) */
int mtg_boss_ctor_build_chunk_dist(mtg_boss_ctor *ctor, mtg_comm *comm, mtg_boss_chunk *out);
/* the same on device-resident reads */
int mtg_boss_build_device_dist(mtg_boss_ctor *ctor, mtg_comm *comm, const uint8_t *d_seq,
                               uint64_t seq_len, const uint64_t *d_read_starts,
                               const uint32_t *d_counts, uint64_t n_reads, void *stream,
                               mtg_boss_device_chunk *out);
/* the range split: bounds[0..world] over n_prefixes buckets, balanced on hist (host) */
int mtg_dist_bounds(const uint64_t *hist, uint64_t n_prefixes, int world, uint64_t *bounds);
/* the identity a rank all-gathers to count the ranks sharing its GPU: a hash of the host name (or
   MTG_HOST_ID) and the device's PCI bus id; and that count for `rank` over every rank's identity
   (timings' coresident; the ranks on one GPU split its free HBM when they plan rounds) */
uint64_t mtg_device_identity(const char *host, const char *pci_bus_id);
uint32_t mtg_dist_coresident(const uint64_t *ids, int world, int rank);

/*
 * The graph files `metagraph build` writes from a chunk (cli/build.cpp:323-352; DBGSuccinct::serialize,
 * dbg_succinct.cpp:754-790): <outbase>.dbg (BOSS F / k / state, W, last, the graph mode, the
 * suffix-range index), <outbase>.edgemask with mask_dummy (1 = --mask-dummy: the valid edges of
 * mark_all_dummy_edges, dbg_succinct.cpp:839-870; 2 = concatenate --clear-dummy: the redundant
 * source dummies of suffix chunks erased first, boss.cpp:1443-1650, and no weights file, as
 * build_boss_from_chunks takes none), <outbase>.dbg.weights when the chunk has
 * weights (node_weights.cpp:62-68).  graph_mode: 0 basic, 1 canonical.  suffix_length < 0 = the
 * build's default min(10, k).  *n_valid (may be NULL) = edges left valid by the mask (`nodes (k)` of
 * `metagraph stats`), else n - 1.  Host code: needs no device.  The sdsl-lite containers inside
 * (wt_huff<> for W, bit_vector_stat for last, bit_vector_small for the mask, int_vector<> for the
 * weights) are written field by field as sdsl-lite 2.x serializes them (csrc/sdsl_io.hpp, DESIGN.md
 * §9); no reference-written file exists to pin their bytes.
 */
int mtg_boss_write_dbg(const mtg_boss_chunk *chunk, const char *outbase, int graph_mode, int mask_dummy,
                       int64_t suffix_length, uint64_t *n_valid);

/*
 * The same files from a chunk in device memory, bit for bit what mtg_boss_write_dbg writes from the
 * same arrays copied to the host.  `chunk` is any device chunk on the constructor's device: the
 * descriptor mtg_boss_build_device[_dist] returned, or arrays the caller uploaded (W and last one byte
 * per row, weights u32 per row or NULL).  The arrays are only read and stay valid; the call takes the
 * constructor's mutex, runs on its stream and frees its device scratch before it returns.  The per-row
 * stages (W's wavelet-tree bits, the rank words, the suffix-range index, the valid-edge mask, the
 * weights' int_vector) run as kernels (csrc/dbg_device.hpp); the Huffman shape, the select supports,
 * bit_vector_small and the framing stay host code.  <outbase>.dbg.weights is written when weights !=
 * NULL and bits_per_count != 0.  mask_dummy: 0 or 1; 2 (pruning) returns MTG_ERR_UNSUPPORTED here: call
 * mtg_boss_write_dbg_device_pruned below (or copy the chunk to the host and use mtg_boss_write_dbg).  A
 * row with W >= 16 returns MTG_ERR_ARGUMENT before any file is written.  graph_mode, suffix_length and
 * *n_valid as for mtg_boss_write_dbg.
 */
typedef struct mtg_dbg_write_timings {
    double device_ms;    /* kernels, events on the constructor's stream */
    double d2h_ms;       /* payload copies to pinned host blocks */
    double host_ms;      /* select supports, bit_vector_small, framing, file writes */
    uint64_t d2h_bytes;
} mtg_dbg_write_timings;
int mtg_boss_write_dbg_device(mtg_boss_ctor *ctor, const mtg_boss_device_chunk *chunk,
                              uint8_t bits_per_count, const char *outbase, int graph_mode,
                              int mask_dummy, int64_t suffix_length, uint64_t *n_valid,
                              mtg_dbg_write_timings *timings /* may be NULL */);

/*
 * `concatenate --clear-dummy` from a chunk in device memory: the device counterpart of mtg_boss_write_dbg
 * with mask_dummy = 2, bit for bit.  The redundant source dummies of the concatenated suffix chunks are
 * found and erased on the device (csrc/dbg_prune.hpp: the single-incoming flags, the source-dummy tree
 * walked down level by level and reduced back up, BOSS::erase_edges as a compaction), then <outbase>.dbg
 * and <outbase>.edgemask are written from the pruned arrays, and no weights file.  The chunk's arrays are
 * only read; mutex, stream and scratch as for mtg_boss_write_dbg_device.  *n_valid, *n_erased (the rows
 * the pruning removed) and timings may be NULL.  Arrays that are no BOSS table (a source-dummy tree that
 * outgrows the rows) return MTG_ERR_ARGUMENT before any file is written.
 */
int mtg_boss_write_dbg_device_pruned(mtg_boss_ctor *ctor, const mtg_boss_device_chunk *chunk,
                                     const char *outbase, int graph_mode, int64_t suffix_length,
                                     uint64_t *n_valid, uint64_t *n_erased,
                                     mtg_dbg_write_timings *timings /* may be NULL */);

/*
 * BOSS::erase_edges (boss.cpp:1342-1403) alone, on the device: the rows of `in` with d_erase[i] == 0 go
 * to `out` in order.  An erased row's `last` moves to the previous kept row (not to row 0), a minus label
 * c + 5 whose class lost a plain c since its previous kept row becomes c, F counts the kept rows.
 * d_erase: one byte per row on the device, row 0 must be 0.  out->W and out->last are caller-allocated
 * device arrays of in->n bytes, distinct from the input's; out->k, out->n and out->F are filled, weights
 * are not carried.  `in` is only read.
 */
int mtg_boss_erase_edges_device(mtg_boss_ctor *ctor, const mtg_boss_device_chunk *in, const uint8_t *d_erase,
                                mtg_boss_device_chunk *out);

/*
 * BOSS::Chunk::extend (boss_chunk.cpp:230-270) on caller-owned device arrays of dst_capacity_rows rows:
 * rows 1.. of src are appended to dst with device-to-device copies, F, n_real and n_dummy are summed; a
 * src of one row is a no-op.  A dst of no rows (n == 0) takes src whole.  A constructor's own device
 * chunk lives until its next build: extend each suffix chunk into such a buffer, then prune the buffer.
 * MTG_ERR_ARGUMENT when k differs, when the capacity is too small, or when exactly one side has weights.
 */
int mtg_boss_chunk_extend_device(mtg_boss_ctor *ctor, mtg_boss_device_chunk *dst, uint64_t dst_capacity_rows,
                                 const mtg_boss_device_chunk *src);

/*
 * The unitigs of a chunk in device memory with their k-mer counts: BOSS::call_unitigs (boss.cpp:2921-3015)
 * over call_paths with split_to_unitigs (boss.cpp:2042-2236), filtered as `metagraph clean` filters them, all
 * on the device (csrc/unitigs.hpp).  A k-mer is a real edge of the chunk (no source dummy, no sink); a unitig
 * is a maximal chain of k-mers u -> v where v is the only k-mer after u and u the only k-mer before v; every
 * k-mer lies in exactly one unitig.  A chain that closes on itself starts at its smallest row.  Records come
 * in ascending row of their first k-mer, so the output is deterministic (the reference's order depends on its
 * threads).  A unitig of m k-mers is a record of m + k chars (upper-case ACGT; k = the chunk's BOSS k) with
 * its m weights in path order.
 *   min_tip_size t: a unitig of fewer than t k-mers is dropped when it is a dead end, by call_unitigs' rule:
 *     kept when its last k-mer has two or more successors, else kept when its first k-mer has two or more
 *     predecessors, else dropped when the last has no successor, else dropped when the first has no
 *     predecessor, else kept.
 *   min_median_abundance a (is_unreliable_unitig, graph_cleaning.cpp:14-32): a unitig is dropped when more
 *     than half of its k-mers weigh less than a.
 * Both filters are evaluated on the unfiltered graph, in one pass.
 * `seq` (records back to back, one '$' after each), `record_starts` (n_records + 1 entries) and
 * `kmer_counts` are exactly what mtg_kmer_counts_to_reads_device (record starts + counts) and
 * mtg_boss_build_device (the buffer) accept: build -> clean -> rebuild without leaving the device.  A chunk
 * with no real edge gives zero records.  The chunk's arrays are only read; mutex, stream (NULL = the
 * constructor's own) and scratch as for the device writers.  Free `out` with mtg_device_unitigs_free.
 * On return the call has synchronised `stream` (the record and k-mer totals are host values), the three
 * arrays are complete, and the constructor's own stream is restored whatever the return code.
 * The chunk must be a full construction or a pruned table: the unpruned concatenation of suffix chunks,
 * whose redundant source dummies change the in-degrees, is not covered.  Not built: kmers_in_single_form
 * (a canonical chunk yields the unitigs of both strands), call_sequences (contigs), --smoothing-window and
 * the count-quantile slices of `clean`.
 * MTG_ERR_ARGUMENT: NULL arguments, min_median_abundance > 1 on a chunk without weights.
 * MTG_ERR_UNSUPPORTED: a chunk of 2^32 rows or more (the links are 32-bit).
 */
typedef struct mtg_unitig_params {
    uint64_t min_tip_size;          /* 0 and 1: keep everything */
    uint64_t min_median_abundance;  /* <= 1: off; > 1 needs weights, else MTG_ERR_ARGUMENT */
} mtg_unitig_params;

typedef struct mtg_device_unitigs {
    uint8_t  *seq;            /* records back to back, one '$' after each; device */
    uint64_t  seq_len;
    uint64_t *record_starts;  /* n_records + 1 */
    uint32_t *kmer_counts;    /* n_kmers entries or NULL (no weights) */
    uint64_t  n_records, n_kmers;
    uint64_t  n_dropped_records, n_dropped_kmers;   /* by the two filters */
    int device_id;
} mtg_device_unitigs;

int mtg_boss_unitigs_device(mtg_boss_ctor *ctor, const mtg_boss_device_chunk *chunk,
                            const mtg_unitig_params *params /* NULL = defaults: 1, 1 */, void *stream,
                            mtg_device_unitigs *out);
void mtg_device_unitigs_free(mtg_device_unitigs *unitigs);
/* doubling rounds the ranking of the constructor's last mtg_boss_unitigs_device /
   mtg_boss_write_unitigs_device call took (ceil(log2(longest unitig)) + 1, more with closed chains) */
uint64_t mtg_boss_unitigs_last_rounds(const mtg_boss_ctor *ctor);

/*
 * The same unitigs written as the pair ExtendedFastaWriter writes (seq_io/sequence_io.cpp:91-183) and
 * mtg_boss_ctor_add_fasta_counts reads: base = outbase without a trailing ".gz" and then without ".fasta";
 * base.fasta.gz holds '>' + the record's 1-based number, a line end, the sequence on one line; with weights
 * base.kmer_counts.gz holds a u32 k-mer length (k + 1), then the u32 counts in record order; both through
 * zlib.  Without weights only the FASTA is written.  The three arrays go to pinned blocks of the host pool
 * first.  `stats` (may be NULL) receives the counts, its pointers stay NULL.  Argument errors return before a
 * file is opened; a file that cannot be written leaves none behind.
 */
int mtg_boss_write_unitigs_device(mtg_boss_ctor *ctor, const mtg_boss_device_chunk *chunk,
                                  const mtg_unitig_params *params, const char *outbase,
                                  mtg_device_unitigs *stats);

/* One sdsl-lite container of the graph files written alone to `path` (the layout tests): kind 0
 * bit_vector_stat over `nbits` bits of `data`, 1 bit_vector_small (sd_vector or rrr_vector<63>,
 * whichever predict_size picks), 2 wt_huff<> over `nbits` bytes of `data`, 3 the sd_vector<> of the
 * set bits, 4 rrr_vector<63>. */
int mtg_sdsl_write(const char *path, int kind, const void *data, uint64_t nbits);

typedef struct mtg_dbg_file {
    uint64_t k;
    uint64_t n;                  /* rows incl. row 0 */
    uint64_t F[5];
    uint64_t state;              /* 3 = STAT */
    uint64_t mode;               /* 0 basic, 1 canonical */
    uint64_t suffix_length;
    uint64_t n_ranges;           /* 4^suffix_length */
    uint8_t *W;                  /* n labels */
    uint64_t *last;              /* n bits, packed */
    uint64_t *ranges;            /* 2 * n_ranges: first and last edge of each indexed suffix */
    uint64_t *valid;             /* packed .edgemask bits, NULL when there is none */
    uint64_t n_valid;
} mtg_dbg_file;
int mtg_boss_read_dbg(const char *outbase, mtg_dbg_file *out);
void mtg_dbg_file_free(mtg_dbg_file *file);

/* the library's pool of pinned host blocks (chunk arrays, staged FASTA files): bytes held by spare
   blocks (at most 4 GiB; blocks above that are unpinned when freed), and a trim that unpins them all */
uint64_t mtg_host_pool_bytes(void);
void mtg_host_pool_trim(void);

/* encode table of the extractor (kmer/alphabets.hpp:127-143) evaluated by the device function on
   the host: out[c] in {0, 1, 2, 3, 4 = invalid} for every byte c (256 entries) */
void mtg_dna_encode_table(uint8_t *out);

/* device-memory helpers for callers without their own HIP runtime (ctypes, cgo, JNI) */
void *mtg_device_alloc(int device_id, uint64_t bytes);
int mtg_device_free(void *ptr);
int mtg_memcpy_h2d(void *dst, const void *src, uint64_t bytes);
int mtg_memcpy_d2h(void *dst, const void *src, uint64_t bytes);
int mtg_device_count(void);
/* device-to-device copy of `bytes` (multiple of 16, 16-byte aligned) by a streaming 16-byte-lane
   kernel on `stream` (NULL = default): the bench's achievable-HBM-bandwidth probe */
int mtg_device_copy(void *dst, const void *src, uint64_t bytes, void *stream);
int mtg_device_synchronize(int device_id);

#ifdef __cplusplus
}
#endif

#endif /* MTG_BOSS_H */
