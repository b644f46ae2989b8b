/*
 * ringpop_amd.h — C ABI of librpamd.so, the MI355X-native engine for ringpop-node's
 * data-parallel core (hash ring, SWIM membership merge + checksum, gossip rounds).
 *
 * Drop-in boundary: these are the entry points a Node N-API addon (or any FFI) binds to
 * replace the reference's in-process hot path. Each function names the reference
 * interface it replaces (paths relative to ringpop v10.9.6). Conventions:
 *   - every function returns 0 on success or a negative status; rp_last_error() gives the
 *     thread-local message. Empty results are NOT errors (reference returns null / []).
 *   - host pointers are borrowed for the duration of the call; *_dev variants take device
 *     pointers and a HIP stream (void*; NULL = the null stream, except rp_wire_decode*_dev,
 *     where NULL = the members handle's own stream) and are stream-ordered. A handle's device
 *     scratch is ordered across streams: a call on another stream than the handle's previous
 *     one first waits for the work queued on that stream. Device-side ordering faults (a
 *     look-back wait that gave up) are reported as RP_EDEVICE at the next host-synchronizing
 *     call on the handle.
 *   - owner ids are interned server ids (stable for the life of a ring); 0xFFFFFFFF = null.
 *   - strings are byte ranges (UTF-8): `bytes` + `off[n+1]` (uint32 offsets) or a fixed
 *     `stride`. Handles are not thread-safe (one HIP stream per handle).
 */
#ifndef RINGPOP_AMD_H
#define RINGPOP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_NULL_ID 0xFFFFFFFFu

/* ------------------------------------------------------------------ common */
const char *rp_last_error(void);
/* Library/ABI version (major<<16 | minor). */
uint32_t rp_version(void);
/* Number of visible HIP devices (0 when none). */
int rp_device_count(int *n);

/* ------------------------------------------------------------------ farmhash32
 * Replaces npm `farmhash` ^0.2.0 hash32 (reference package.json:34), called at
 * lib/ring/index.js:29,55,102,140,146,166 and lib/membership/index.js:65.
 * rp_hash32 is the host C++ implementation (the reference's addon is host C++ too);
 * rp_hash32_batch_dev hashes n device strings (off: n+1 uint64 byte offsets). */
uint32_t rp_hash32(const char *s, size_t len);
int rp_hash32_batch_dev(const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n, uint32_t *d_out,
                        void *stream);
/* farmhash32 of ONE long device string d_bytes[0, len) (the checksum strings of
 * lib/ring/index.js:96-105 and lib/membership/index.js:48-75 are hashed this way): one serial
 * chain fed by producer lanes. d_out[0] = hash (d_out must hold 2 uint32). */
int rp_hash32_long_dev(const uint8_t *d_bytes, uint64_t len, uint32_t *d_out, void *stream);
/* farmhash32 of n long device strings side by side (the membership checksum groups): string b
 * is d_bytes + b * stride; d_meta[4b] = its length + 1 (a builder's piece total), d_meta[4b + 1]
 * = its gate (0: skipped, nothing written); the hash goes to d_meta[4b + 2] and d_meta[4b + 3] =
 * 1. Each string must be readable 12 bytes past its end. 16-B aligned strings at a 16-B multiple
 * stride run kHpStr strings a workgroup (RP_HL_PACK=0: one a workgroup). */
int rp_hash32_long_multi_dev(const uint8_t *d_bytes, uint64_t stride, uint32_t n, uint32_t *d_meta, void *stream);

/* Synthetic key stream: n UUID-v4-format 36-byte keys [k0, k0+n) of `seed`,
 * written at 36-byte stride. */
int rp_gen_uuid_keys_dev(uint32_t seed, uint64_t k0, uint64_t n, uint8_t *d_out, void *stream);

/* ------------------------------------------------------------------ HashRing
 * Replaces lib/ring/index.js HashRing (25-189) and its RBTree (lib/ring/rbtree.js) with a
 * sorted token array in HBM. */
typedef struct rp_ring rp_ring;

/* new HashRing({replicaPoints}) (lib/ring/index.js:25-34); replica_points 0 => 100. */
int rp_ring_create(uint32_t replica_points, int device, rp_ring **out);
int rp_ring_destroy(rp_ring *r);

/* addRemoveServers(serversToAdd, serversToRemove) (lib/ring/index.js:60-94); also the
 * building block of addServer/removeServer (39-48, 124-133). Tokens are farmhash32 of
 * server + String(i) computed on the device, unless add_tokens/rem_tokens (n*R uint32,
 * row j = input server j) carry a caller hashFunc's values (options.hashFunc, :29).
 * *changed_out = ringChanged. The checksum is recomputed on the device when changed. */
int rp_ring_add_remove(rp_ring *r,
                       const char *add_bytes, const uint32_t *add_off, uint32_t n_add,
                       const uint32_t *add_tokens,
                       const char *rem_bytes, const uint32_t *rem_off, uint32_t n_rem,
                       const uint32_t *rem_tokens,
                       int *changed_out);

/* ring.checksum (lib/ring/index.js:33,96-105): farmhash32 of the sorted server names joined
 * by ';'. *is_set = 0 while the reference value would still be null. */
int rp_ring_checksum(rp_ring *r, uint32_t *out, int *is_set);
/* The joined checksum string (for callers with a custom hashFunc): writes up to cap bytes,
 * *len = full length. */
int rp_ring_checksum_string(rp_ring *r, char *buf, uint64_t cap, uint64_t *len);
/* getServerCount (:107-109), rbtree.size, hasServer (:118-120). */
int rp_ring_server_count(rp_ring *r, uint32_t *out);
int rp_ring_token_count(rp_ring *r, uint32_t *out);
int rp_ring_has_server(rp_ring *r, const char *name, uint32_t len, int *out);
/* Interned id of a name (RP_NULL_ID if never seen) and id -> name. */
int rp_ring_server_id(rp_ring *r, const char *name, uint32_t len, uint32_t *id);
const char *rp_ring_owner_name(rp_ring *r, uint32_t id, uint32_t *len);
/* Object.keys(servers) in insertion order (getStats, :111-116): ids_out[cap], *n = count. */
int rp_ring_servers(rp_ring *r, uint32_t *ids_out, uint32_t cap, uint32_t *n);
/* Copy the sorted (token, owner) arrays to host (in-order rbtree walk). */
int rp_ring_dump(rp_ring *r, uint32_t *tokens, uint32_t *owners, uint32_t cap);

/* Batched lookup(key) (:145-154) and lookupN(key, n) (:157-189), host buffers in and out
 * (PCIe-inclusive). Keys: stride > 0 => key i = keys[i*stride .. +stride); else
 * keys[off[i] .. off[i+1]) with uint64 offsets. lookupN output rows have max(n,1) slots,
 * unused = RP_NULL_ID; counts (nullable) = result length per key. */
int rp_ring_lookup(rp_ring *r, const char *keys, const uint64_t *off, uint32_t stride, uint64_t n,
                   uint32_t *owners);
int rp_ring_lookupn(rp_ring *r, const char *keys, const uint64_t *off, uint32_t stride, uint64_t n,
                    int32_t nrep, uint32_t *owners, uint8_t *counts);
/* Low-latency single calls (RingPop.lookup / lookupN per request, index.js:434-471): with
 * idle_ms > 0, a one-key rp_ring_lookup / rp_ring_lookupn / rp_ring_lookupn_hashes (n <= 8; the
 * host hashes the key) is answered by a resident service (eight one-wave workgroups, one an XCD,
 * RP_SVC_WAVES) that polls a pinned, device-mapped request line on a staggered schedule and reads
 * one record of its direct table (built at its first launch after a ring change), instead of a
 * kernel launch and a stream sync per call. The waves exit after idle_ms without a
 * request (and after 30 s in all) and is relaunched by the next call; a ring mutation and every
 * other device call on this ring (batch lookups, grouping, dump) stop it first. Every device
 * call of this library on any other handle stops every resident service as well and keeps new
 * ones from starting until it returns (a resident wave would make its hipFree wait, and its
 * stream may share a hardware queue), so no call of the library waits for a wave to idle out;
 * device work queued outside the library is not covered. idle_ms = 0 (the default) turns it
 * off. */
int rp_ring_service(rp_ring *r, uint32_t idle_ms);
/* Same with precomputed key hashes (hashFunc(key) done by the caller). */
int rp_ring_lookup_hashes(rp_ring *r, const uint32_t *hashes, uint64_t n, uint32_t *owners);
int rp_ring_lookupn_hashes(rp_ring *r, const uint32_t *hashes, uint64_t n, int32_t nrep,
                           uint32_t *owners, uint8_t *counts);
/* Device-resident forms (the hot path): inputs already in HBM, stream-ordered, no sync. */
int rp_ring_lookup_dev(rp_ring *r, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                       uint64_t n, uint32_t *d_owners, void *stream);
int rp_ring_lookupn_dev(rp_ring *r, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                        uint64_t n, int32_t nrep, uint32_t *d_owners, uint8_t *d_counts, void *stream);
int rp_ring_lookupn_hashes_dev(rp_ring *r, const uint32_t *d_hashes, uint64_t n, int32_t nrep,
                               uint32_t *d_owners, uint8_t *d_counts, void *stream);

/* Keys grouped by owner: RingPop.handleOrProxyAll's keysByDest = _.groupBy(keys, this.lookup)
 * (index.js:609-667, :616) and RequestProxySend.lookupKeys (lib/request-proxy/send.js:171-179).
 * Every key is looked up (lib/ring/index.js:145-154); on an empty ring every key gets self_id
 * (RingPop.lookup's whoami() fallback, index.js:434-451). Outputs:
 *   dests[0 .. *ndest)        the distinct owners in first-seen order = Object.keys(keysByDest)
 *                             (lookupKeys' result); capacity min(n, server_count + 1)
 *   group_off[0 .. *ndest]    group g holds perm[group_off[g] .. group_off[g+1])
 *   perm[0 .. n)              key indices; each group keeps input order (keysByDest[dest])
 * The _dev form takes device buffers (group_off holding n + 1) and never syncs with the host
 * unless the ring is empty. */
int rp_ring_group_keys_dev(rp_ring *r, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride, uint64_t n,
                           uint32_t self_id, uint32_t *d_dests, uint32_t *d_group_off, uint32_t *d_perm,
                           uint32_t *d_ndest, void *stream);
int rp_ring_group_keys(rp_ring *r, const char *keys, const uint64_t *off, uint32_t stride, uint64_t n,
                       uint32_t self_id, uint32_t *dests, uint32_t *group_off, uint32_t *perm, uint32_t *ndest);
/* Same with a caller hashFunc's key hashes (options.hashFunc, lib/ring/index.js:29). */
int rp_ring_group_hashes(rp_ring *r, const uint32_t *hashes, uint64_t n, uint32_t self_id, uint32_t *dests,
                         uint32_t *group_off, uint32_t *perm, uint32_t *ndest);

/* Ring snapshots: an immutable device copy of the ring's exact lookup arrays (sorted tokens,
 * owners, bucket index) as of the call, with the token count, server count and checksum of that
 * moment. A snapshot owns its memory and holds no pointer into the ring: it stays valid across
 * any number of later rp_ring_add_remove calls and may be destroyed before or after the ring.
 * Its owner ids are the ring's interned ids (stable for the life of the ring; resolve names with
 * rp_ring_owner_name on the ring). A snapshot of an empty ring is legal. rp_ring_snapshot is a
 * device call on r (it stops a resident service and is ordered after pending rebuilds). */
typedef struct rp_ring_snap rp_ring_snap;
int rp_ring_snapshot(rp_ring *r, rp_ring_snap **out);
int rp_ring_snap_destroy(rp_ring_snap *s);
int rp_ring_snap_info(const rp_ring_snap *s, uint32_t *token_count, uint32_t *server_count,
                      uint32_t *checksum, int *checksum_is_set);
/* lookupN under the snapshotted ring: the rows rp_ring_lookupn_dev wrote at snapshot time
 * (answering under the old ring, e.g. the request proxy's checksum-mismatch case). */
int rp_ring_snap_lookupn_dev(rp_ring_snap *s, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                             uint64_t n, int32_t nrep, uint32_t *d_owners, uint8_t *d_counts, void *stream);

/* Moved keys: which keys changed hands between a snapshot and the ring now (hand-off after
 * ringChanged). Key i has moved iff its lookupN(key, nrep) row under `before` differs from its
 * row under r, compared as ordered lists including their lengths; rows have W = max(nrep, 1)
 * slots padded with RP_NULL_ID, exactly what rp_ring_lookupn* writes (nrep <= 0 keeps lookupn's
 * single-step form). One pass: each key is read and hashed once, both rings are searched from
 * that hash, and rows are written for moved keys only.
 *   *count                    the number of moved keys, counted in full
 *   idx[0 .. min(count,cap))  the moved key indices, ascending (input order)
 *   before_rows / after_rows  [j*W .. j*W+W): the two rows of key idx[j]; either may be NULL
 * Nothing at or past entry cap is touched (cap = 0: count only; idx may then be NULL).
 * `before` must be a snapshot of a ring on r's device with r's id space (normally of r itself).
 * nrep > 8 and n >= 2^32 return RP_EINVAL (rows are compared in registers, 8 owners at most).
 * The _dev form takes device buffers (d_count one uint32), is stream-ordered and never syncs
 * with the host, except that a stream other than the ring's own first waits for the ring's
 * pending rebuilds (as rp_ring_lookupn_dev does). */
int rp_ring_moved_keys_dev(rp_ring *r, const rp_ring_snap *before,
                           const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride, uint64_t n,
                           int32_t nrep, uint32_t cap,
                           uint32_t *d_idx, uint32_t *d_before, uint32_t *d_after, uint32_t *d_count,
                           void *stream);
int rp_ring_moved_keys(rp_ring *r, const rp_ring_snap *before, const char *keys, const uint64_t *off,
                       uint32_t stride, uint64_t n, int32_t nrep, uint32_t cap,
                       uint32_t *idx, uint32_t *before_rows, uint32_t *after_rows, uint32_t *count);
/* Same with a caller hashFunc's key hashes (options.hashFunc, lib/ring/index.js:29). */
int rp_ring_moved_hashes(rp_ring *r, const rp_ring_snap *before, const uint32_t *hashes, uint64_t n,
                         int32_t nrep, uint32_t cap, uint32_t *idx, uint32_t *before_rows,
                         uint32_t *after_rows, uint32_t *count);

/* Owner load and hash-space share: how many keys each server carries, as primary and as the 2nd
 * to n-th replica, and which share of the 2^32 hash values it owns (the expected load).
 * One past the largest server id this ring has interned (ids of removed servers included). */
int rp_ring_id_bound(rp_ring *r, uint32_t *out);

/* Owner load: load[id * W + q] = number of keys whose lookupN(key, nrep) row has server `id` in
 * slot q; W = max(nrep, 1). The rows are exactly what rp_ring_lookupn* writes. RP_NULL_ID
 * padding is not counted. load has id_cap * W entries. id_cap < rp_ring_id_bound is RP_EINVAL
 * with nothing written. accumulate = 0: load is overwritten. Nonzero: the counts are added to
 * what load holds, so a key set can be fed in batches. Any n (uint64). Any nrep that
 * rp_ring_lookupn_dev accepts. An empty ring counts nothing.
 * The keys are looked up in chunks of RP_LOAD_CHUNK keys (default 2^24) into a scratch the handle
 * owns (chunk * W * 4 bytes, whatever n is), and each chunk's rows are counted on the same
 * stream. The _dev form is stream-ordered and never syncs with the host, except that a stream
 * other than the ring's own first waits for the ring's pending rebuilds (as rp_ring_lookupn_dev
 * does). */
int rp_ring_owner_load_dev(rp_ring *r, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                           uint64_t n, int32_t nrep, uint32_t id_cap, int accumulate,
                           uint64_t *d_load, void *stream);
int rp_ring_owner_load(rp_ring *r, const char *keys, const uint64_t *off, uint32_t stride, uint64_t n,
                       int32_t nrep, uint32_t id_cap, uint64_t *load);          /* host buffers, overwrites */
int rp_ring_owner_load_hashes(rp_ring *r, const uint32_t *hashes, uint64_t n, int32_t nrep,
                              uint32_t id_cap, uint64_t *load);                 /* caller hashFunc */
/* The same under a snapshot's ring (ids are the ring's interned ids; the id bound is the ring's
 * at snapshot time). The snapshot allocates its row scratch at first use. */
int rp_ring_snap_owner_load_dev(rp_ring_snap *s, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                                uint64_t n, int32_t nrep, uint32_t id_cap, int accumulate,
                                uint64_t *d_load, void *stream);

/* Hash-space share: share[id] = how many of the 2^32 hash values h have lookup(h) == id
 * (lib/ring/index.js:145-154: the first token >= h, else the smallest token). The shares sum to
 * 2^32 on a non-empty ring and are all 0 on an empty one. Host output, id_cap entries.
 * id_cap is checked as above. */
int rp_ring_owner_share(rp_ring *r, uint32_t id_cap, uint64_t *share);
int rp_ring_snap_owner_share(rp_ring_snap *s, uint32_t id_cap, uint64_t *share);

/* Moved ranges: which hash intervals changed hands between a snapshot and the ring now, without
 * any key (range hand-off of stores indexed by hash; planning a ring change before keys exist).
 * For a hash h, row_S(h) is the row rp_ring_lookupn_hashes writes for h under ring state S with
 * nrep: W = max(nrep, 1) slots padded with RP_NULL_ID (nrep <= 0 keeps lookupn's single-step
 * form, so a hash above the last token then has an empty row). The moved set is
 * {h in [0, 2^32) : row_before(h) != row_after(h)}. The result is its unique decomposition into
 * maximal runs of consecutive hash values on which the pair (row_before, row_after) is constant,
 * ascending by lo. Runs do not wrap: a run that ends at 2^32-1 and one that starts at 0 are two
 * entries even when their rows are equal.
 *   lo[j], hi[j]              the run, both ends inclusive
 *   before_rows / after_rows  [j*W .. j*W+W): the two rows of run j; either may be NULL
 *   *count                    the number of runs, counted in full
 *   *moved_hashes             the size of the moved set, counted in full (it can be 2^32)
 * Nothing at or past entry cap is touched (cap = 0: the counts only; the arrays may then be NULL).
 * count is at most tokens_before + tokens_now + 1: both rows are constant between neighbours of
 * the sorted union of both token sets with 2^32-1 appended, so a cap of that size holds every run.
 * `before` must be a snapshot of a ring on r's device with r's id space (normally of r itself), as
 * for rp_ring_moved_keys. nrep > 8 (rows are compared in registers), a null handle and a snapshot
 * on another device return RP_EINVAL with nothing written.
 * The _dev forms take device buffers (d_count one uint32, d_moved_hashes one uint64, 8-byte
 * aligned), are stream-ordered and never sync with the host, except that a stream other than the
 * ring's own first waits for the ring's pending rebuilds (as rp_ring_moved_keys_dev does). Their
 * scratch (13 bytes per token of either side) belongs to the handle and is allocated when it
 * first grows, never per call after that. */
int rp_ring_moved_ranges_dev(rp_ring *r, const rp_ring_snap *before, int32_t nrep, uint32_t cap,
                             uint32_t *d_lo, uint32_t *d_hi, uint32_t *d_before, uint32_t *d_after,
                             uint32_t *d_count, uint64_t *d_moved_hashes, void *stream);
int rp_ring_moved_ranges(rp_ring *r, const rp_ring_snap *before, int32_t nrep, uint32_t cap,
                         uint32_t *lo, uint32_t *hi, uint32_t *before_rows, uint32_t *after_rows,
                         uint32_t *count, uint64_t *moved_hashes);
/* The same between two snapshots of one ring (after owns the scratch, allocated at first use). */
int rp_ring_snap_moved_ranges_dev(const rp_ring_snap *before, rp_ring_snap *after, int32_t nrep, uint32_t cap,
                                  uint32_t *d_lo, uint32_t *d_hi, uint32_t *d_before, uint32_t *d_after,
                                  uint32_t *d_count, uint64_t *d_moved_hashes, void *stream);
int rp_ring_snap_moved_ranges(const rp_ring_snap *before, rp_ring_snap *after, int32_t nrep, uint32_t cap,
                              uint32_t *lo, uint32_t *hi, uint32_t *before_rows, uint32_t *after_rows,
                              uint32_t *count, uint64_t *moved_hashes);
/* The snapshot's sorted (token, owner) arrays, as rp_ring_dump gives them for a ring. */
int rp_ring_snap_dump(const rp_ring_snap *s, uint32_t *tokens, uint32_t *owners, uint32_t cap);

/* Hand-off plan: which keys to send to whom after a ring change (what an application does on
 * ringChanged). For key i let B be its lookupN(key, nrep) row under `before` and A its row under
 * r: exactly the rows rp_ring_moved_keys* compares (W = max(nrep, 1) slots padded with
 * RP_NULL_ID, each side with its own min(nrep, server count), nrep <= 0 keeps lookupn's
 * single-step form). Every server in a key's row holds the key.
 *   src(i)     the first entry of B, in slot order, whose server is in r's server set at call
 *              time (not: in A); RP_NULL_ID if none (an orphan: the key comes from elsewhere)
 *   gained     the non-null A[q] that occur nowhere in B, in slot order
 *   transfers  one record (key = i, dst = A[q], src = src(i), slot = q) per gained entry. A key
 *              whose rows differ but whose A gains nothing (its row only shrank, or only changed
 *              order) is moved for rp_ring_moved_keys and has no record here.
 *   only_src   not RP_NULL_ID: only keys with src(i) == only_src produce records (what this
 *              server has to push). RP_NULL_ID keeps every record, orphans included.
 * The record stream is every record in (key index, slot) order; *count is its full length and
 * the result describes its first T = min(count, cap) records (cap may cut between two records of
 * one key), grouped by destination:
 *   dests[0 .. *ndest)        the distinct dst among those T records, ascending by server id
 *   group_off[0 .. *ndest]    group g is entries [group_off[g], group_off[g+1]) of key_idx / src /
 *                             slot; group_off[*ndest] == T
 *   key_idx / src / slot      per record; inside a group key indices are strictly ascending (a
 *                             key gains a server at most once). src and slot may be NULL.
 * Capacities: dests min(cap, rp_ring_id_bound) entries, group_off one more, key_idx / src / slot
 * cap each; nothing at or past them is touched. Results, not errors: n == 0, an empty ring now
 * (nothing is gained) and cap == 0 (counts only; the arrays may then be NULL) give *ndest = 0 and
 * group_off[0] = 0 (where group_off is given); an empty `before` gives every key its whole A with
 * src = RP_NULL_ID. nrep > 8, n * W >= 2^32 (the look-back word carries 32 bits of running
 * count), a null handle, a snapshot on another device, and an only_src that is neither
 * RP_NULL_ID nor below rp_ring_id_bound return RP_EINVAL with nothing written.
 * One pass reads and hashes each key once, searches both rings and writes the record stream to a
 * scratch the ring owns (13 bytes per record slot, allocated when it first grows, never per call
 * after that); a stable radix sort by dst then groups it. The _dev form takes device buffers
 * (d_ndest, d_count one uint32 each), is stream-ordered and never syncs with the host, except
 * that a stream other than the ring's own first waits for the ring's pending rebuilds (as
 * rp_ring_moved_keys_dev does). It cannot know the record count on the host, so its grouping
 * passes run over min(cap, n * W) slots: their cost follows cap. Size cap from a count-only call
 * (cap = 0) or from the moved share (rp_ring_moved_ranges) rather than from n * W. The host forms
 * read the count back after the first pass and group exactly T records. */
int rp_ring_handoff_dev(rp_ring *r, const rp_ring_snap *before,
                        const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride, uint64_t n,
                        int32_t nrep, uint32_t only_src, uint32_t cap,
                        uint32_t *d_dests, uint32_t *d_group_off, uint32_t *d_key_idx, uint32_t *d_src,
                        uint8_t *d_slot, uint32_t *d_ndest, uint32_t *d_count, void *stream);
int rp_ring_handoff(rp_ring *r, const rp_ring_snap *before, const char *keys, const uint64_t *off,
                    uint32_t stride, uint64_t n, int32_t nrep, uint32_t only_src, uint32_t cap,
                    uint32_t *dests, uint32_t *group_off, uint32_t *key_idx, uint32_t *src,
                    uint8_t *slot, uint32_t *ndest, uint32_t *count);
/* Same with a caller hashFunc's key hashes (options.hashFunc, lib/ring/index.js:29). */
int rp_ring_handoff_hashes(rp_ring *r, const rp_ring_snap *before, const uint32_t *hashes, uint64_t n,
                           int32_t nrep, uint32_t only_src, uint32_t cap,
                           uint32_t *dests, uint32_t *group_off, uint32_t *key_idx, uint32_t *src,
                           uint8_t *slot, uint32_t *ndest, uint32_t *count);

/* Routing agreement: every key's owner under many views of one ring at once (what handleOrProxy
 * does with ring.lookup(key) on nodes whose rings differ while gossip spreads). r is the base
 * ring: it holds every server. A view allows a subset of its servers. For a key hash h let i be
 * the position of the first token >= h, wrapping to 0, as lookup finds it
 * (lib/ring/index.js:145-154). Then
 *   owner(v, h)  the owner of the first token in i, i + 1, ... (cyclic, at most every token once)
 *                whose server view v allows; RP_NULL_ID if there is none.
 * That is lookup on a ring holding exactly the view's servers as long as no two servers' replica
 * tokens collide. Where tokens collide (about 108 of 10^6 at 10,000 servers) the answer is
 * defined by this walk over r's arrays; the reference's insert-if-absent / erase-by-key rings
 * depend on their history there. lookup only (n = 1).
 * Inputs:
 *   keys         d_keys with d_off / stride as for rp_ring_lookup_dev, or d_hashes (a caller
 *                hashFunc's key hashes): exactly one of d_keys and d_hashes is given
 *   views        server id is allowed in view v when it has a token in r, col = d_col[id] is not
 *                RP_NULL_ID, and d_rows[v * row_stride + col] & bit is non-zero. d_col NULL:
 *                col = id, and then row_stride >= id_cap. A col at or past row_stride counts as
 *                RP_NULL_ID. d_col has id_cap entries; id_cap >= rp_ring_id_bound, else RP_EINVAL.
 *   d_truth      one more view, the truth: d_truth[col] & bit. NULL: every server of r. t(k) is
 *                key k's owner under the truth.
 *   d_active     d_active[v] != 0 marks the views that are counted. NULL: all.
 * Outputs, each nullable:
 *   wrong[v]         keys with owner(v, k) != t(k)
 *   lost[v]          keys whose owner(v, k) is not null and is not allowed by the truth (requests
 *                    sent to a server that is gone); lost[v] <= wrong[v]
 *                    Both are uint64[n_views]. accumulate != 0 adds to what they hold, otherwise
 *                    they are set; inactive views get 0 (are left alone under accumulate).
 *   key_wrong[k]     active views with owner(v, k) != t(k)
 *   truth_owner[k]   t(k)
 *   owners[k * n_views + v]  owner(v, k) of every view, active or not (the diagnostic output:
 *                    4 * n * n_views bytes)
 * n == 0 and n_views == 0 are not errors. The planes (n_views bits per server id) live in a
 * scratch the ring owns, allocated when it first grows, never per call after that. A view that
 * allows S_v of S servers costs about S / S_v walk steps per key, in that view's word only: a
 * view with one server out of thousands walks up to every token per key. The _dev form is
 * stream-ordered and never syncs with the host, except that a stream other than the ring's own
 * first waits for the ring's pending rebuilds (as rp_ring_lookupn_dev does). The host form takes
 * host buffers (truth: row_stride bytes) and is synchronous. */
int rp_ring_route_views_dev(rp_ring *r, const uint8_t *d_keys, const uint64_t *d_off, uint32_t stride,
                            const uint32_t *d_hashes, uint64_t n,
                            const uint8_t *d_rows, uint64_t row_stride, uint8_t bit, uint32_t n_views,
                            const uint32_t *d_col, uint32_t id_cap,
                            const uint8_t *d_truth, const uint8_t *d_active, int accumulate,
                            uint64_t *d_wrong, uint64_t *d_lost, uint32_t *d_key_wrong,
                            uint32_t *d_truth_owner, uint32_t *d_owners, void *stream);
int rp_ring_route_views(rp_ring *r, const char *keys, const uint64_t *off, uint32_t stride,
                        const uint32_t *hashes, uint64_t n,
                        const uint8_t *rows, uint64_t row_stride, uint8_t bit, uint32_t n_views,
                        const uint32_t *col, uint32_t id_cap,
                        const uint8_t *truth, const uint8_t *active, int accumulate,
                        uint64_t *wrong, uint64_t *lost, uint32_t *key_wrong,
                        uint32_t *truth_owner, uint32_t *owners);

/* Routing agreement over the hash space, without keys: on how many of the 2^32 hash values each
 * view disagrees with the truth. It is to rp_ring_route_views what rp_ring_moved_ranges is to
 * rp_ring_moved_keys and rp_ring_owner_share to rp_ring_owner_load: exact, deterministic and
 * independent of any key set. With tok[0 .. M) / own[0 .. M) the ring's sorted arrays
 * (rp_ring_dump), the interval of position i is the set of hashes whose lookup position is i:
 * (tok[i-1], tok[i]] for i > 0, and [0, tok[0]] together with (tok[M-1], 2^32-1] for i = 0. Its
 * length len(i) is what rp_ring_owner_share adds: tok[i] - tok[i-1], and tok[0] + 2^32 - tok[M-1]
 * for i = 0 (2^32 on a one-token ring); the lengths sum to 2^32. owner(v, h) and t(h) are as
 * rp_ring_route_views documents them and are constant on every interval, where they equal their
 * value at h = tok[i]; owner(v, i), t(i) below. Views, d_col, bit, row_stride, id_cap, d_truth
 * (NULL: every server of r) and d_active mean exactly what they mean there.
 * Outputs, each nullable:
 *   wrong[v]      the sum of len(i) over the positions with owner(v, i) != t(i)
 *   lost[v]       the sum of len(i) over the positions where owner(v, i) is not null and is not
 *                 allowed by the truth; lost[v] <= wrong[v] <= 2^32
 *                 Both are uint64[n_views]. accumulate != 0 adds to what they hold, otherwise they
 *                 are set; inactive views get 0 (are left alone under accumulate).
 *   pos_wrong[i]  active views with owner(v, i) != t(i), uint32 by token position: where in the
 *                 hash space the views disagree. Always set, never accumulated. pos_cap is the
 *                 buffer's capacity in entries and covers the token count (rp_ring_token_count),
 *                 else RP_EINVAL. With rp_ring_dump it gives the disputed share of the hash
 *                 space: the sum of len(i) over the positions with pos_wrong[i] > 0.
 * Results, not errors: n_views == 0; an empty ring (everything 0, nothing is written to
 * pos_wrong); a truth that allows nobody (t is null everywhere: a view is wrong and lost on all
 * 2^32 hashes iff it allows anybody). RP_EINVAL with nothing written: a null handle, bit == 0,
 * id_cap below rp_ring_id_bound, without d_col a row_stride below id_cap, pos_wrong with pos_cap
 * below the token count, more views than rp_ring_route_views takes. Token collisions need no
 * extra rule: r's arrays hold distinct tokens, and the walk over them is the definition.
 * The cost is (tokens) x (n_views / 64) wave steps whatever the views and the truth look like: a
 * sparse truth or a one-server view costs no more (the wrong / lost bits of position i follow
 * from those of i + 1 by a generate / propagate recurrence, which is scanned in chunks; DESIGN
 * §4.2g). RP_SHARE_CHUNK (read once per call) sets the positions a chunk. The planes and the
 * chunk aggregates live in the ring's routing scratch, allocated when it first grows, never per
 * call after that. The _dev form is stream-ordered and never syncs with the host, except that a
 * stream other than the ring's own first waits for the ring's pending rebuilds (as
 * rp_ring_route_views_dev does). The host form takes host buffers (truth: row_stride bytes) and
 * is synchronous. */
int rp_ring_route_share_dev(rp_ring *r, const uint8_t *d_rows, uint64_t row_stride, uint8_t bit,
                            uint32_t n_views, const uint32_t *d_col, uint32_t id_cap,
                            const uint8_t *d_truth, const uint8_t *d_active, int accumulate,
                            uint64_t *d_wrong, uint64_t *d_lost, uint32_t *d_pos_wrong, uint32_t pos_cap,
                            void *stream);
int rp_ring_route_share(rp_ring *r, const uint8_t *rows, uint64_t row_stride, uint8_t bit,
                        uint32_t n_views, const uint32_t *col, uint32_t id_cap,
                        const uint8_t *truth, const uint8_t *active, int accumulate,
                        uint64_t *wrong, uint64_t *lost, uint32_t *pos_wrong, uint32_t pos_cap);

/* ------------------------------------------------------------------ Membership
 * Replaces the hot path of lib/membership/index.js Membership: update (249-324) with the
 * Member.evaluateUpdate rules (lib/membership/member.js:71-202) and computeChecksum /
 * generateChecksumString (48-75, 100-123). Members are interned address ids; status codes
 * 0 alive, 1 suspect, 2 faulty, 3 leave (member.js:204-209). The JS wrapper keeps the
 * Member objects, the members array order (getJoinPosition, 129-131) and the isReady stash
 * (259-265): call update only where the reference would evaluate (ready or isLocal). */
typedef struct rp_members rp_members;

int rp_members_create(uint32_t capacity, int device, rp_members **out);
int rp_members_destroy(rp_members *m);
/* Intern addresses (ids_out[i] for each; existing names keep their id). */
int rp_members_intern(rp_members *m, const char *bytes, const uint32_t *off, uint32_t n, uint32_t *ids_out);
/* whoami(): the local member's id (local override, member.js:155-169). */
int rp_members_set_local(rp_members *m, uint32_t local_id);
/* Membership.update(changes) for k changes (ids, status, incarnation) evaluated in array order
 * with Date.now() = now_ms. applied[i]: 0 not applied, 1 applied, 2 created a new member;
 * new_status/new_inc: the update as applied (local override rewrites it). If anything applied
 * the checksum is recomputed once. Host buffers (all outputs nullable). Incarnations must lie in
 * [-2^60, 2^60) (a JS Number is exact to 2^53; the member table stores 61 bits) and statuses in
 * 0..3, else RP_EINVAL with nothing applied. */
int rp_members_update(rp_members *m, const uint32_t *ids, const uint8_t *status, const int64_t *inc, uint32_t k,
                      int64_t now_ms, uint8_t *applied, uint8_t *new_status, int64_t *new_inc,
                      uint32_t *n_applied);
/* Same, device buffers, stream-ordered, no host synchronization (d_n_applied nullable). An
 * incarnation outside [-2^60, 2^60) is reported as RP_EDEVICE by the handle's next host-
 * synchronizing call. The status / incarnation outputs may be the input arrays themselves (the
 * reference rewrites its update objects in place): the copy is then skipped. */
int rp_members_update_dev(rp_members *m, const uint32_t *d_ids, const uint8_t *d_status, const int64_t *d_inc,
                          uint32_t k, int64_t now_ms, uint8_t *d_applied, uint8_t *d_new_status,
                          int64_t *d_new_inc, uint32_t *d_n_applied, void *stream);
/* The merge partitioned by member id (lib/membership/index.js:249-324 split by id):
 * the same update over device buffers, applied only to the changes whose id lies in [id_lo,
 * id_hi) (whole buckets of 4,096 ids; id_hi may be the capacity). Those changes are evaluated in
 * array order as update_dev would; the outputs (applied, new status / incarnation) of the other
 * changes are left as they were, *d_n_applied counts this range's applied changes, and rows
 * outside the range are not touched. No checksum is computed: a caller holding the table in
 * ranges brings the rows together (rp_members_rows_copy) and calls rp_members_compute_checksum.
 * Always the bucket path (no damp scoring, at most 8M ids); a range past the table folds nothing
 * (*d_n_applied = 0). Stream-ordered, no host sync. */
int rp_members_update_range_dev(rp_members *m, const uint32_t *d_ids, const uint8_t *d_status,
                                const int64_t *d_inc, uint32_t k, int64_t now_ms, uint32_t id_lo, uint32_t id_hi,
                                uint8_t *d_applied, uint8_t *d_new_status, int64_t *d_new_inc,
                                uint32_t *d_n_applied, void *stream);
/* The member rows of ids [id_lo, id_hi) (8 B each: incarnation << 3 | exists << 2 | status) to
 * (into_table = 0) or from (1) a device buffer, on `stream`. */
int rp_members_rows_copy(rp_members *m, void *d_buf, uint32_t id_lo, uint32_t id_hi, int into_table, void *stream);
/* membership.checksum (null until the first applied update: *is_set = 0). */
/* Membership.set (lib/membership/index.js:208-247) over the stash of k changes received while
 * not ready (arrival order; the caller keeps the stash, index.js:259-265):
 * mergeMembershipChangesets (lib/membership/merge.js:22-51: the local member skipped, the
 * strictly greatest incarnation per address wins, the first one on ties), then every picked
 * change is set verbatim (existing members overwritten, unknown addresses created), then the
 * checksum is computed once. pick (k entries) receives the indices of the picked changes in
 * first-seen address order (the order the caller appends new Member objects in), npick their
 * count. The _dev form takes device buffers and never syncs with the host. */
int rp_members_set(rp_members *m, const uint32_t *ids, const uint8_t *status, const int64_t *inc, uint32_t k,
                   uint32_t *pick, uint32_t *npick);
int rp_members_set_dev(rp_members *m, const uint32_t *d_ids, const uint8_t *d_status, const int64_t *d_inc,
                       uint32_t k, uint32_t *d_pick, uint32_t *d_npick, void *stream);
int rp_members_checksum(rp_members *m, uint32_t *out, int *is_set);
/* computeChecksum() unconditionally. */
int rp_members_compute_checksum(rp_members *m);
/* defer != 0: update no longer recomputes the checksum after each batch (the reference does,
 * index.js:306-309); a caller folding many batches calls rp_members_compute_checksum once at the
 * end. Default off. */
int rp_members_defer_checksum(rp_members *m, int defer);
/* Batch-strided checksums over replicas (§8e membership merge on G GPUs: every replica folds
 * every batch, so each holds the whole table; the checksum strings and their serial farmhash
 * chains, index.js:48-75 / 306-309, are divided among the replicas). From this call on, update
 * batch b (counting update calls with k > 0 from 0) builds and hashes its checksum only when
 * b % nshards == shard. With history_cap > 0 each such batch's {checksum, applied-anything} is
 * recorded in order (at most history_cap of them; rp_members_checksum_history reads them). A
 * batch that applied nothing leaves the reference's checksum unchanged: a reader carries the
 * previous batch's value forward. nshards = 1, shard = 0 restores the default. */
int rp_members_checksum_shard(rp_members *m, uint32_t nshards, uint32_t shard, uint32_t history_cap);
/* The recorded per-batch checksums (this shard's batches, in batch order): hash[i], applied[i]
 * (0: the batch applied nothing; hash[i] is then 0), up to cap; *n = entries recorded. */
int rp_members_checksum_history(rp_members *m, uint32_t *hash, uint8_t *applied, uint32_t cap, uint32_t *n);
/* Drop the first `count` recorded entries (after reading them), so a long-running replica keeps
 * recording: update refuses a batch with RP_ESTATE, before applying anything, when its entry
 * would not fit history_cap. */
int rp_members_checksum_history_drain(rp_members *m, uint32_t count);
/* generateChecksumString() (writes up to cap bytes; *len = full length). */
int rp_members_checksum_string(rp_members *m, char *buf, uint64_t cap, uint64_t *len);
/* Member table by id (exists/status/incarnation), cap entries. */
int rp_members_dump(rp_members *m, uint8_t *exists, uint8_t *status, int64_t *inc, uint32_t cap);
int rp_members_count(rp_members *m, uint32_t *n_names);

/* ---- flap-damping scores ----
 * Member.dampScore / lastUpdateDampScore / lastUpdateTimestamp (lib/membership/member.js:28-41)
 * kept on the device by member id. Once configured, every update() applies _applyUpdatePenalty
 * (member.js:98-107, 133-153: decay, + penalty, clamp, suppress-limit check) to each applied
 * update of another member at now_ms, stamps lastUpdateTimestamp on every applied update, and
 * gives created members (update() or set()) the initial score; rp_members_damp_decay is
 * Membership._decayMembersDampScore (lib/membership/index.js:374-383) over every member. The
 * fields mirror config.js:60-71; the defaults are {1, 0, 0, 10000, 500, 5000, 60}. The decay
 * factor is V8's Math.pow (fdlibm) restated bit for bit. */
typedef struct rp_damp_config {
    int enabled;            /* dampScoringEnabled: penalize applied updates */
    double initial;         /* dampScoringInitial */
    double min;             /* dampScoringMin */
    double max;             /* dampScoringMax */
    double penalty;         /* dampScoringPenalty */
    double suppress_limit;  /* dampScoringSuppressLimit */
    double half_life;       /* dampScoringHalfLife, seconds (> 0) */
} rp_damp_config;

/* Turn tracking on (first call: every id starts at `initial`, null timestamp) or change the
 * config. Call it where the reference constructs Membership (initMembership, index.js:399-418). */
int rp_members_damp_configure(rp_members *m, const rp_damp_config *cfg);
/* The last update batch, per change in batch order: the member's dampScore after the change and
 * whether 'suppressLimitExceeded' fired (member.js:141-152). k <= that batch's size; an empty
 * batch (k = 0) is a batch too, so after one any k > 0 is RP_EINVAL. */
int rp_members_damp_last(rp_members *m, double *score, uint8_t *exceeded, uint32_t k);
/* The decayer tick at Date.now() = now_ms (host form syncs; _dev is stream-ordered). */
int rp_members_damp_decay(rp_members *m, int64_t now_ms);
int rp_members_damp_decay_dev(rp_members *m, int64_t now_ms, void *stream);
/* Per id (cap entries, nullable outputs): dampScore, lastUpdateDampScore, lastUpdateTimestamp
 * (0 = null). */
int rp_members_damp_dump(rp_members *m, double *score, double *last_score, int64_t *last_ts, uint32_t cap);

/* ------------------------------------------------------------------ Gossip wire bodies
 * Change records as the JSON text ringpop sends (addresses are ids interned in the members
 * handle m). Replaces the per-message JSON.stringify / safeParse of:
 *   issueAs record  {id, source, sourceIncarnationNumber, address, status, incarnationNumber}
 *                   (lib/gossip/dissemination.js:163-170)                                form 0
 *   fullSync record {source, address, status, incarnationNumber} (dissemination.js:64-73)  form 1
 * and the bodies around them (RP_WIRE_BODY_*):
 *   ARRAY             the bare changes array
 *   PING              {checksum, changes, source, sourceIncarnationNumber}  lib/gossip/ping-sender.js:71-76
 *   PING_RESPONSE     {changes}                                              server/protocol/ping.js:45-48
 *   PINGREQ           {checksum, changes, source, sourceIncarnationNumber, target}
 *                                                                    lib/gossip/ping-req-sender.js:75-81
 *   PINGREQ_RESPONSE  {changes, pingStatus, target}                     server/protocol/ping-req.js:61-65
 *   JOIN_RESPONSE     {app, coordinator, membership, membershipChecksum}  server/protocol/join.js:128-133
 *                     (membership = the fullSync records; coordinator = the source column,
 *                     membershipChecksum = the checksum column, app = one string for the batch)
 * JSON.stringify leaves an undefined member out; per record: an ids row whose first byte is NUL,
 * a src of RP_NULL_ID, a src_inc of INT64_MIN (or a null column) are absent and not written.
 * Message j holds records [msg_rec_off[j], msg_rec_off[j+1]): msg_rec_off[0] = 0, not
 * decreasing, msg_rec_off[n_msgs] = n_rec. Every id and offset is validated on the device before
 * anything is written (RP_EINVAL otherwise). Encode writes d_out_off[0..n_msgs] (byte offsets);
 * with d_out null only the offsets are computed (size query). Synchronous. */
enum {
    RP_WIRE_BODY_ARRAY = 0,
    RP_WIRE_BODY_PING = 1,
    RP_WIRE_BODY_PING_RESPONSE = 2,
    RP_WIRE_BODY_PINGREQ = 3,
    RP_WIRE_BODY_PINGREQ_RESPONSE = 4,
    RP_WIRE_BODY_JOIN_RESPONSE = 5
};
typedef struct rp_wire_records {  /* n_rec entries each */
    const uint32_t *addr, *src;     /* member ids (src: RP_NULL_ID = absent) */
    const uint8_t *status;          /* 0 alive 1 suspect 2 faulty 3 leave */
    const int64_t *inc, *src_inc;   /* incarnationNumber; sourceIncarnationNumber (INT64_MIN / null = absent) */
    const uint8_t *ids;             /* 36-byte uuids per record, nullable */
} rp_wire_records;
typedef struct rp_wire_headers {  /* n_msgs entries each, as the body needs them */
    const uint32_t *checksum;       /* PING, PINGREQ: checksum; JOIN_RESPONSE: membershipChecksum */
    const uint32_t *source;         /* PING, PINGREQ: source; JOIN_RESPONSE: coordinator */
    const int64_t *source_inc;      /* PING, PINGREQ: sourceIncarnationNumber */
    const uint32_t *target;         /* PINGREQ, PINGREQ_RESPONSE: target */
    const uint8_t *ping_status;     /* PINGREQ_RESPONSE: pingStatus (0 / 1) */
    const char *app;                /* JOIN_RESPONSE: app (host string, app_len bytes, no escapes) */
    uint32_t app_len;
} rp_wire_headers;
int rp_wire_encode_dev(rp_members *m, uint32_t n_msgs, const uint32_t *d_msg_rec_off, uint64_t n_rec,
                       const rp_wire_records *d_recs, int form, int body, const rp_wire_headers *d_hdr,
                       uint8_t *d_out, uint64_t *d_out_off, void *stream);
/* Host-buffer form (staged through the handle's device; PCIe-bound; ids checked on the host):
 * out NULL = size query (out_off filled); otherwise cap >= out_off[n_msgs]. */
int rp_wire_encode(rp_members *m, uint32_t n_msgs, const uint32_t *msg_rec_off, const rp_wire_records *recs,
                   int form, int body, const rp_wire_headers *hdr, uint8_t *out, uint64_t cap, uint64_t *out_off);

/* Decode n_msgs JSON texts buf[msg_off[j] .. msg_off[j+1]) — a changes array, or a body object
 * whose `changes` (join response: `membership`) member is one; any key order, JSON whitespace,
 * unknown members skipped (server/protocol/ping.js:27-36 reads the same members). msg_rec_off[0..n_msgs]
 * gets record offsets (total in [n_msgs]); records beyond rec_cap are counted, not written. Per
 * record: address id (RP_NULL_ID if not interned; addr_off / addr_len give its bytes), source id
 * (RP_NULL_ID: absent or not interned), status, incarnationNumber, sourceIncarnationNumber
 * (INT64_MIN if absent), byte offset of `id` (~0 if absent). Per message: checksum /
 * membershipChecksum, source / coordinator, sourceIncarnationNumber, target, pingStatus (0xFF if
 * absent); err[j] = 0, or 1 + the failing byte's offset in message j (its records are then
 * dropped). Strings with escapes and non-integral numbers are rejected (addresses and uuids
 * never hold one). Every column except addr / status / inc is nullable. */
typedef struct rp_wire_records_out {
    uint32_t *addr, *src;
    uint8_t *status;
    int64_t *inc, *src_inc;
    uint64_t *id_off, *addr_off;
    uint32_t *addr_len;
} rp_wire_records_out;
typedef struct rp_wire_headers_out {
    uint32_t *checksum, *source;
    int64_t *source_inc;
    uint32_t *target;
    uint8_t *ping_status;
} rp_wire_headers_out;
int rp_wire_decode_dev(rp_members *m, const uint8_t *d_buf, const uint64_t *d_msg_off, uint32_t n_msgs,
                       uint32_t *d_msg_rec_off, uint32_t rec_cap, const rp_wire_records_out *d_recs,
                       const rp_wire_headers_out *d_hdr, uint64_t *d_err, void *stream);
int rp_wire_decode(rp_members *m, const char *buf, const uint64_t *msg_off, uint32_t n_msgs, uint32_t *msg_rec_off,
                   uint32_t rec_cap, const rp_wire_records_out *recs, const rp_wire_headers_out *hdr, uint64_t *err);

/* The first round's column-list forms of the same codec (bodies 0..2). */
int rp_wire_encode_changes_dev(rp_members *m, uint32_t n_msgs, const uint32_t *d_msg_rec_off, uint64_t n_rec,
                               const uint32_t *d_addr, const uint32_t *d_src, const uint8_t *d_status,
                               const int64_t *d_inc, const int64_t *d_src_inc, const uint8_t *d_ids, int form,
                               int body, const uint32_t *d_msg_checksum, const uint32_t *d_msg_source,
                               const int64_t *d_msg_source_inc, uint8_t *d_out, uint64_t *d_out_off, void *stream);
int rp_wire_encode_changes(rp_members *m, uint32_t n_msgs, const uint32_t *msg_rec_off, const uint32_t *addr,
                           const uint32_t *src, const uint8_t *status, const int64_t *inc, const int64_t *src_inc,
                           const uint8_t *ids, int form, int body, const uint32_t *msg_checksum,
                           const uint32_t *msg_source, const int64_t *msg_source_inc, uint8_t *out, uint64_t cap,
                           uint64_t *out_off);
int rp_wire_decode_changes_dev(rp_members *m, const uint8_t *d_buf, const uint64_t *d_msg_off, uint32_t n_msgs,
                               uint32_t *d_msg_rec_off, uint32_t rec_cap, uint32_t *d_addr, uint32_t *d_src,
                               uint8_t *d_status, int64_t *d_inc, int64_t *d_src_inc, uint64_t *d_id_off,
                               uint64_t *d_addr_off, uint32_t *d_addr_len, uint64_t *d_err,
                               uint32_t *d_msg_checksum, uint32_t *d_msg_source, int64_t *d_msg_source_inc,
                               void *stream);
int rp_wire_decode_changes(rp_members *m, const char *buf, const uint64_t *msg_off, uint32_t n_msgs,
                           uint32_t *msg_rec_off, uint32_t rec_cap, uint32_t *addr, uint32_t *src, uint8_t *status,
                           int64_t *inc, int64_t *src_inc, uint64_t *err);

/* ------------------------------------------------------------------ Gossip simulator
 * N full ringpop nodes (every node: membership view, dissemination buffer, ring membership,
 * iterator, suspicion timers; lib/membership, lib/gossip, lib/ring, lib/on_membership_event.js)
 * advanced in the deterministic round model of DESIGN.md §SWIM round model: ping / ping-req
 * exchange, piggyback counters with maxPiggybackCount, suspect->faulty timers. No reference
 * counterpart (the reference is one view per process). names/off: N member addresses;
 * inc0[N]: initial incarnations (every view starts identical, all alive); dead[N]: members
 * killed before round 0. seed: Philox seed of the iterator shuffles and ping-req samples;
 * suspicion_rounds: 5000 ms / 200 ms = 25 by default; now0: Date.now() at round 0. */
typedef struct rp_sim rp_sim;

int rp_sim_create(uint32_t n, const char *names, const uint32_t *off, const int64_t *inc0, const uint8_t *dead,
                  uint32_t seed, uint32_t suspicion_rounds, int64_t now0, int device, rp_sim **out);
int rp_sim_destroy(rp_sim *s);
/* Advance `rounds` rounds (synchronous) / enqueue them (asynchronous, rp_sim_sync waits). */
int rp_sim_step(rp_sim *s, uint32_t rounds);
int rp_sim_step_async(rp_sim *s, uint32_t rounds);
int rp_sim_sync(rp_sim *s);
int rp_sim_round(rp_sim *s, int64_t *out);
/* Every node's membership checksum (0 for killed nodes). */
int rp_sim_checksums(rp_sim *s, uint32_t *out);
/* Node v's view: status[N], incarnation[N] (nullable). */
int rp_sim_view(rp_sim *s, uint32_t v, uint8_t *status, int64_t *inc);
/* Convergence (scenario-runner.js:152-170): all live checksums equal and every killed member
 * faulty in every live view. */
int rp_sim_converged(rp_sim *s, int *out);
/* pings, ping-reqs, full syncs, applied updates since creation. */
int rp_sim_stats(rp_sim *s, uint64_t *out4);

/* ---- Sharded simulator (C5): a handle owns the nodes [bounds[shard], bounds[shard+1]) of a
 * partition of [0, n) into nshards contiguous ranges (bounds NULL = equal ranges); its views
 * still cover all n members. A round is five stages (rp_sim_stage 0..4) separated by four
 * message exchanges: after stage k < 4 the outbox holds this shard's messages grouped by
 * destination shard (rp_sim_outbox: per-destination message / record counts and ONE device
 * buffer holding, for each destination in shard order, a segment of its 40-byte headers then
 * its 24-byte records); before stage k + 1 the caller fills the inbox (rp_sim_inbox sizes it for
 * the per-source counts and returns its device buffer) with every source's segment for this
 * shard, in source-shard order — one all-to-all-v moves the bytes as they lie. The buffers are
 * owned by the handle and valid until its next stage. Neither call waits for the device (round
 * 6): the counts are on the host when rp_sim_stage returns, but the outbox bytes are written, and
 * the inbox is still read by the previous stage, on the handle's stream. Before reading the
 * outbox or writing the inbox the caller orders itself after that stream with
 * rp_sim_order_stream (a device stream waits on the device; NULL: the host waits). rp_sim_exchange_local does the
 * exchange for handles of one process; across processes the host moves the bytes (RCCL
 * all-to-all-v; ringpop-node_amd DistGossipSim). Checksums / views / stats are per shard
 * (checksums: the shard's nodes in id order); convergence reduces rp_sim_converged_local
 * {live nodes, min checksum, max checksum, killed-not-faulty flag} over the shards. */
int rp_sim_create_shard(uint32_t n, const char *names, const uint32_t *off, const int64_t *inc0, const uint8_t *dead,
                        uint32_t seed, uint32_t suspicion_rounds, int64_t now0, int device, const uint32_t *bounds,
                        uint32_t nshards, uint32_t shard, rp_sim **out);
int rp_sim_shard_info(rp_sim *s, uint32_t *v0, uint32_t *nl, uint32_t *nshards, uint32_t *shard);
int rp_sim_stage(rp_sim *s, int stage);
int rp_sim_outbox(rp_sim *s, uint64_t *nmsg, uint64_t *nrec, void **buf);
int rp_sim_inbox(rp_sim *s, const uint64_t *nmsg, const uint64_t *nrec, void **buf);
/* The handle's next stage waits (on the device, no host sync) for the work queued so far on
 * `stream`: a caller that moved the inbox bytes with a collective on its own stream (RCCL on
 * torch's stream) orders the import after it this way. */
int rp_sim_wait_stream(rp_sim *s, void *stream);
/* The converse: `stream` waits (on the device) for the work queued so far on the handle's stream;
 * stream NULL: the host waits for it. */
int rp_sim_order_stream(rp_sim *s, void *stream);
int rp_sim_exchange_local(rp_sim *const *shards, uint32_t nshards);
int rp_sim_converged_local(rp_sim *s, uint32_t *out4);
/* JOIN events on a sharded simulator (a joiner reads its responders' views, which other shards
 * may hold). Before rp_sim_stage(s, 0) of every round, on every shard, repeat until *has == 0:
 * rp_sim_join_export applies the round's events up to its next join, runs the join handler of
 * the responders this shard owns and returns a device buffer of *bytes bytes holding their
 * rows (zeros elsewhere; every byte has exactly one writing shard). The caller combines the
 * shards' buffers into each shard's own buffer by a byte-wise sum (an RCCL / gloo all-reduce of
 * uint8, or rp_sim_join_exchange_local for handles in one process), then calls
 * rp_sim_join_import, which builds the joiner's view on its shard. (Replaces the responders'
 * join handler + the joiner's mergeJoinResponses / set(): server/protocol/join.js:126,
 * join-response-merge.js:40-56, membership/index.js:208-247.) */
int rp_sim_join_export(rp_sim *s, int *has, void **buf, uint64_t *bytes);
int rp_sim_join_import(rp_sim *s);
int rp_sim_join_exchange_local(rp_sim *const *shards, uint32_t nshards);

/* ---- Scenarios. Events run before phase A of their round, in the order given:
 *   RP_SIM_KILL    the node goes down (crash / SIGSTOP, scripts/tick-cluster.js:417-470): it
 *                  neither acts nor answers; its state is kept
 *   RP_SIM_REVIVE  it comes back with that state (SIGCONT)
 *   RP_SIM_LEAVE   the admin leave (server/admin/member.js:70-98): makeLeave(whoami, own
 *                  incarnation) (lib/membership/index.js:191-195), as the convergence scenarios
 *                  send it (benchmarks/convergence-time/scenarios/); its LocalMemberLeaveEvent
 *                  stops the node's gossip loop and suspicion (on_membership_event.js:32-40). A
 *                  node that is down ignores it, and so does one whose own status is `leave`
 *                  (a node that left and then refuted a suspicion is alive and leaves again).
 *   RP_SIM_JOIN    a fresh process for the node bootstraps into the running cluster
 *                  (index.js:240-322): makeAlive(self, Date.now()); three live nodes, or the one
 *                  or two there are (JOIN Philox stream over the live nodes in id order), answer
 *                  the join
 *                  (server/protocol/join.js:126-133: makeAlive(joiner), fullSync);
 *                  mergeJoinResponses (join-response-merge.js:40-56) is stashed and set()
 *                  (index.js:208-247) builds the view, the set handler
 *                  (on_membership_event.js:42-67) fills the ring and the suspicion timers; the
 *                  dissemination is cleared as at bootstrap, then gossip.start shuffles. Needs one
 *                  live node besides the joiner: with nobody to answer, the reference's join
 *                  never completes, and the step (or rp_sim_join_export) that reaches the event
 *                  fails with RP_EINVAL. A sharded handle takes joins through rp_sim_join_export /
 *                  rp_sim_join_import.
 *   RP_SIM_SIDE    the node moves to side `reserved` (0..255, else RP_EINVAL) of the network.
 *                  side[N] is one byte a node, 0 for everyone at creation, global on every shard.
 *                  A sender v reaches u when u is up and side[v] == side[u]; a node across the cut
 *                  is to v exactly what a down node is: it gets no ping, gives no answer and
 *                  cannot help a ping-req (a helper v reaches is on v's side and cannot reach v's
 *                  target either, so pingStatus stays false). It differs from a down node only in
 *                  running its own rounds on its side. A partition is a batch of these in one
 *                  round. Kill, revive, leave and join keep the node's side; a join is answered
 *                  by live nodes on the joiner's side (none: RP_EINVAL, as above).
 *   RP_SIM_HEAL    every node's side becomes 0 (`node` is ignored; it must still be < n).
 *                  Message loss, one-way links and delays are not modelled.
 * `reserved` is read only by RP_SIM_SIDE. Convergence is global, with or without a cut, and reads: every node that is up and has not left holds the same checksum, each
 * member that left is `leave` and each other member that is down `faulty` in those views.
 * dead[] = down from the start (never started gossip; gossip/index.js:97 never shuffled). */
typedef struct rp_sim_event {
    uint32_t round, kind, node, reserved;
} rp_sim_event;
enum { RP_SIM_KILL = 0, RP_SIM_REVIVE = 1, RP_SIM_LEAVE = 2, RP_SIM_JOIN = 3, RP_SIM_SIDE = 4, RP_SIM_HEAL = 5 };
int rp_sim_create_scenario(uint32_t n, const char *names, const uint32_t *off, const int64_t *inc0,
                           const uint8_t *dead, uint32_t seed, uint32_t suspicion_rounds, int64_t now0, int device,
                           const uint32_t *bounds, uint32_t nshards, uint32_t shard, const rp_sim_event *events,
                           uint32_t n_events, rp_sim **out);
/* Every local node's dissemination.maxPiggybackCount (dissemination.js:38-55), [shard nodes]. */
int rp_sim_piggyback(rp_sim *s, uint32_t *out);
/* Traffic since creation: {pings, ping-reqs, full syncs, applied updates, messages sent, change
 * records sent, views hashed, bytes of the all-alive checksum string (a view's string length
 * within a few bytes per deviated member)}. */
int rp_sim_counters(rp_sim *s, uint64_t *out8);
/* Node v's ring membership: in_ring[N] 0/1, what its ring holds (kept by the alive / faulty /
 * leave handler and the join's set handler, lib/on_membership_event.js). */
int rp_sim_ring_members(rp_sim *s, uint32_t v, uint8_t *in_ring);
/* Every local node's ring checksum (lib/ring/index.js:96-105 computeChecksum), out[the handle's
 * nodes] in id order: farmhash32 of the names of the members node v's ring holds (the rows with
 * rp_sim_ring_members' bit), in address order (Object.keys(servers).sort() of ASCII addresses),
 * joined by ';' with no trailing separator. It is the value a forwarded request's head carries
 * (lib/request-proxy/send.js:135-147) and the receiver compares with its own
 * (lib/request-proxy/index.js:168-191), NOT the membership checksum of rp_sim_checksums: a suspect
 * member stays in the ring, so views with different membership checksums can share a ring checksum.
 * A ring that holds nobody gives hash32("") = 0xdc56d17a, computed on the host. A node that is
 * down answers too: its ring is kept, as its rows are. On the handle's stream after the rounds
 * queued so far, host output, synchronous; a sharded handle answers only at a round boundary
 * (before stage 0), else RP_EINVAL; an empty shard writes nothing. Computed on demand: no round
 * does anything for it. The call scans every node's deviation bitmap (only the status bytes of set
 * bits are read, by the invariant rp_sim_census documents), describes each view by (absent members,
 * their name bytes, a 64-bit order-free fingerprint of their ranks), and builds and hashes one
 * string per class of equal views: a view whose description equals a lower-id view's is compared
 * with it exactly, word by word, and copies its result only when the absent sets are equal, so a
 * fingerprint collision costs a comparison and never a wrong checksum. RP_SIM_RCK_TWINS=0 (read
 * per call; default on) builds every view. The strings are built in batches into a scratch the
 * handle owns, of at most RP_SIM_RCK_BYTES bytes (read per call; default 256 MB, at least one
 * string), and hashed by the launcher of rp_hash32_long_multi_dev. */
int rp_sim_ring_checksums(rp_sim *s, uint32_t *out);
/* Routing agreement of the handle's nodes: rp_ring_route_views_dev on the handle's stream, after
 * the rounds queued so far, with every local node's ring membership as one view of `ring`. ring
 * holds the members as servers, matched by name (a member the ring lacks is allowed nowhere; the
 * map is cached per ring handle and id bound) and lives on the handle's device, else RP_EINVAL.
 * truth[a] != 0: member a really serves; node v is counted when truth[v] != 0. truth NULL on an
 * unsharded handle: the node is up (neither dead[] nor killed by the scenario so far) and its
 * own status in its own view is not `leave`. A sharded handle needs truth (RP_EINVAL otherwise)
 * and routes only at a round boundary (before stage 0). Host buffers, synchronous; outputs as
 * rp_ring_route_views documents them, each nullable: wrong / lost [the handle's nodes],
 * key_wrong / truth_owner [n] (truth_owner: ring ids). */
int rp_sim_routing(rp_sim *s, rp_ring *ring, const char *keys, const uint64_t *off, uint32_t stride, uint64_t n,
                   const uint8_t *truth, uint64_t *wrong, uint64_t *lost, uint32_t *key_wrong,
                   uint32_t *truth_owner);
int rp_sim_routing_hashes(rp_sim *s, rp_ring *ring, const uint32_t *hashes, uint64_t n, const uint8_t *truth,
                          uint64_t *wrong, uint64_t *lost, uint32_t *key_wrong, uint32_t *truth_owner);
/* The same without keys, exact over the hash space: rp_ring_route_share_dev on the handle's
 * stream with the same views, truth and counted nodes as rp_sim_routing (same rules for the ring's
 * device, the default truth and sharded handles). Host buffers, synchronous; outputs as
 * rp_ring_route_share documents them, each nullable: wrong / lost [the handle's nodes] in hash
 * values of the 2^32, pos_wrong [the ring's token count <= pos_cap] by token position (the shards'
 * pos_wrong add up). */
int rp_sim_routing_share(rp_sim *s, rp_ring *ring, const uint8_t *truth,
                         uint64_t *wrong, uint64_t *lost, uint32_t *pos_wrong, uint32_t pos_cap);
/* Census of every member over the handle's views, on the handle's stream after the rounds queued
 * so far. Observers O: the handle's nodes v with observe[v] != 0 (observe: uint8[N], global, by
 * node id); observe NULL: every local node that is up now (the nodes rp_sim_checksums reports a
 * checksum for). A node that is down may be observed explicitly: its view is kept. With st_v(a),
 * inc_v(a), ring_v(a) node v's row for member a, the outputs, by member id and each nullable:
 *   n_obs            |O|
 *   status[a*4 + s]  #{v in O : st_v(a) = s}, s = alive, suspect, faulty, leave   [N*4]
 *   in_ring[a]       #{v in O : ring_v(a)}                                       [N]
 *   max_inc[a]       max over v in O of inc_v(a); INT64_MIN when O is empty       [N]
 *   at_max[a]        #{v in O : inc_v(a) = ref[a]}                               [N]
 *   behind[lv]       for v in O: #{a : inc_v(a) < ref[a]}; 0 outside O           [the handle's nodes]
 * ref = max_ref[N] when given, else this call's own max_inc. No shard of a sharded simulator sees
 * the global maximum: the host takes the element-wise max of the shards' max_inc and passes it
 * back as max_ref (status, in_ring and at_max then add up over the shards). A sharded handle
 * answers only at a round boundary (before stage 0), else RP_EINVAL. An empty shard or an empty O
 * gives zeros and INT64_MIN. Host buffers, synchronous; the scratch belongs to the handle and is
 * reused. The rows are not swept: the call reads every node's deviation bitmap ([W] words by
 * address rank) and only the rows whose bit is set, because a clear bit means the row is still
 * (alive, inc0[a], in the ring). Three places keep that: the bootstrap clears the bitmap
 * (k_sim_init), every row update sets the bit next to its store (block_apply), and a join
 * rebuilds the joiner's bitmap by the same rule (k_join_view); no other code writes a row.
 * at_max and behind cost a second pass over the bitmap, made only when one of them is asked for.
 * RP_CENSUS_ROWS (read per call) sets the rows a workgroup covers. */
int rp_sim_census(rp_sim *s, const uint8_t *observe, const int64_t *max_ref, uint32_t *n_obs, uint32_t *status,
                  uint32_t *in_ring, int64_t *max_inc, uint32_t *at_max, uint32_t *behind);
/* Every node's side of the network now (the RP_SIM_SIDE / RP_SIM_HEAL events applied so far):
 * side[N], global, the same on every shard. */
int rp_sim_sides(rp_sim *s, uint8_t *side);
/* Convergence per side, on the handle's stream after the rounds queued so far. Observers: the
 * handle's nodes that rp_sim_converged compares (up and not left). Four arrays of 256 entries by
 * side id, each nullable:
 *   nodes[s]           observers on side s
 *   ck_min[s], ck_max[s]  the range of their checksums; 0xFFFFFFFF and 0 where nodes[s] == 0
 *   cross_pingable[s]  #{(observer v on s, member a) : a is down or on another side, and v holds a
 *                      as alive or suspect} (Member.isPingable)
 * A side has settled when ck_min == ck_max and cross_pingable == 0. Over the shards of a sharded
 * simulator nodes and cross_pingable add up and the min / max combine; a sharded handle answers
 * only at a round boundary (before stage 0), else RP_EINVAL. Host buffers, synchronous; the scratch
 * belongs to the handle. Two launches: the count and range (one wave reduction per side present in
 * a wave), then a sweep of the observers' status rows, one wave a row, made only when
 * cross_pingable is asked for. */
int rp_sim_side_summary(rp_sim *s, uint32_t *nodes, uint32_t *ck_min, uint32_t *ck_max, uint64_t *cross_pingable);

/* ---- Timeline: what happened, round by round, recorded on the device. While it is enabled every
 * round ends (stage 4) by appending one record of cluster-wide aggregates to a ring of records on
 * the handle's stream, with no wait of the host, so one read after rp_sim_step_async(R) returns R
 * records. st_v(a), ring_v(a): observer v's row for member a. */
typedef struct rp_sim_round_rec {   /* 128 bytes, 8-byte aligned, unused tail zero */
    uint64_t round;          /* the round that just ended (0-based: the record of the first step of a
                                fresh handle is round 0) */
    uint32_t observers;      /* the handle's nodes rp_sim_converged compares: up and not left */
    uint32_t ck_min, ck_max; /* range of their checksums; 0xFFFFFFFF and 0 when observers == 0 */
    uint32_t reserved;
    uint64_t pairs[4];       /* #(observer v, member a) by st_v(a): alive, suspect, faulty, leave;
                                they sum to observers * N */
    uint64_t in_ring;        /* #(observer v, member a) with ring_v(a) */
    uint64_t unmet;          /* sum over the members convergence wants at a status (left -> leave, other
                                down members -> faulty) of the observers NOT holding them there */
    uint64_t false_faulty;   /* #(observer v, member a): a is itself up and has not left, and v holds it
                                faulty or leave (a live server missing from v's ring) */
    uint64_t stats[4];       /* pings, ping-reqs, full syncs, applied updates since creation (rp_sim_stats)
                                as of the end of this round */
    uint64_t tail[2];        /* zero */
} rp_sim_round_rec;
/* The observers and the wanted statuses are rp_sim_converged's, after the round's events, so
 *   observers == 0 || (ck_min == ck_max && unmet == 0)
 * is what rp_sim_converged (one shard; sharded: the reduction of rp_sim_converged_local) would have
 * answered after that round. Over the shards of one simulator observers, pairs, in_ring, unmet,
 * false_faulty and stats add up and ck_min / ck_max combine by min / max; that is why unmet is a
 * count and not a flag.
 * rp_sim_timeline_enable: cap > 0 records from the next round on and keeps the last cap rounds;
 * it resets everything (records and first_seen become 0xFFFFFFFF), also when the timeline was
 * already on. cap == 0 turns recording off and frees the buffers. The buffers (cap * 128 B of
 * records, n * 3 * 4 B of first_seen, n * 5 * 4 B of per-rank counters, n * 2 B of flags) belong to
 * the handle and are allocated here, never per round. A sharded handle takes the call only at a
 * round boundary (before stage 0), else RP_EINVAL and nothing changes. RP_TIMELINE_ROWS (read
 * here) sets the rows a workgroup of the bitmap pass covers. A handle that never enables the
 * timeline launches, copies and waits for nothing new.
 * rp_sim_timeline_read waits for the handle's stream as rp_sim_sync does (with its error check)
 * and copies the kept records oldest first: *n = min(rounds recorded since enable, cap, cap_out),
 * the newest ones when cap_out is the smaller; *first_round = out[0].round. The host knows both
 * from its own round counter. first_seen[a*3 + (s-1)] (uint32 [n*3], nullable), s = suspect,
 * faulty, leave: the first recorded round at whose end some observer held member a at status s,
 * 0xFFFFFFFF if none did; the ring's wrapping does not touch it, and over shards it combines by
 * min. Timeline off: *n = 0 and first_seen is left alone, no error. A sharded handle answers only
 * at a round boundary (before stage 0), else RP_EINVAL.
 * Cost of a recorded round: the refresh the next round's stage 0 would have run (that stage then
 * finds nothing to hash unless events dirty views), the observer count of rp_sim_converged written
 * into the record, one pass over the observers' deviation bitmaps gathering only the status byte
 * of set bits (the census's tiling), and one thread per address rank folding the counters into
 * the record.
 * Not given, on purpose: a per-member round at which EVERY observer held a status (not a
 * reduction of per-shard values; rp_sim_census answers it at any chosen round) and a per-side
 * timeline (rp_sim_side_summary answers per side at any chosen round). */
int rp_sim_timeline_enable(rp_sim *s, uint32_t cap);
int rp_sim_timeline_read(rp_sim *s, rp_sim_round_rec *out, uint32_t cap_out, uint32_t *n, uint64_t *first_round,
                         uint32_t *first_seen);

/* Stream-ordered copy between any host / device buffers (hipMemcpyDefault); NULL stream =
 * synchronous. Used by hosts that move sharded-simulator messages. */
int rp_copy(void *dst, const void *src, uint64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
