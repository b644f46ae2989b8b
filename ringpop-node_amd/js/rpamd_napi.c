/*
 * rpamd_napi.c — Node N-API addon over librpamd.so (include/ringpop_amd.h).
 *
 * This is the "thin Node N-API C-ABI addon calling HIP" of BASELINE.json north_star: it
 * only marshals JS values into the C ABI's plain buffers; every hash, sort, lookup, merge and
 * gossip round runs in librpamd's HIP kernels. There is no JS or CPU fallback — a missing
 * library or device raises. The JS classes that mirror the reference's API (lib/ring/index.js
 * HashRing, Membership.update, farmhash.hash32) are in index.js next to this file.
 *
 * Built by ./Makefile (gcc, N-API v3+ headers of the node in this image, rpath to ..).
 */
#include <node_api.h>
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ringpop_amd.h"

/* ------------------------------------------------------------------ helpers */
#define NAPI_OK(call)                                                                 \
    do {                                                                              \
        if ((call) != napi_ok) {                                                      \
            const napi_extended_error_info *ei_ = NULL;                               \
            napi_get_last_error_info(env, &ei_);                                      \
            napi_throw_error(env, NULL, ei_ && ei_->error_message ? ei_->error_message \
                                                                  : "napi call failed"); \
            return NULL;                                                              \
        }                                                                             \
    } while (0)

#define RP_OK(call)                                                \
    do {                                                           \
        if ((call) != 0) {                                         \
            napi_throw_error(env, "ERR_RINGPOP_AMD", rp_last_error()); \
            return NULL;                                           \
        }                                                          \
    } while (0)

#define ARGS(N)                                                            \
    size_t argc = (N);                                                     \
    napi_value argv[(N) > 0 ? (N) : 1];                                    \
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));         \
    if (argc < (N)) {                                                      \
        napi_throw_type_error(env, NULL, "wrong number of arguments");     \
        return NULL;                                                       \
    }

static int64_t *f64_to_i64(napi_env env, const double *d, size_t n, int nan_is_min, const char *what);

static napi_value make_u32(napi_env env, uint32_t v) {
    napi_value out;
    napi_create_uint32(env, v, &out);
    return out;
}

static napi_value make_bool(napi_env env, int v) {
    napi_value out;
    napi_get_boolean(env, v != 0, &out);
    return out;
}

static napi_value make_null(napi_env env) {
    napi_value out;
    napi_get_null(env, &out);
    return out;
}

static int is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return 1;
    return t == napi_null || t == napi_undefined;
}

/* Handles are napi externals whose finalizer destroys the native object unless destroy()
 * already did (the slot is then NULL). */
typedef struct {
    int kind; /* 1 ring, 2 members, 3 sim, 4 ring snapshot */
    void *p;
} handle_t;

static void handle_finalize(napi_env env, void *data, void *hint) {
    (void)env;
    (void)hint;
    handle_t *h = (handle_t *)data;
    if (h->p) {
        if (h->kind == 1) rp_ring_destroy((rp_ring *)h->p);
        if (h->kind == 2) rp_members_destroy((rp_members *)h->p);
        if (h->kind == 3) rp_sim_destroy((rp_sim *)h->p);
        if (h->kind == 4) rp_ring_snap_destroy((rp_ring_snap *)h->p);
    }
    free(h);
}

static napi_value wrap_handle(napi_env env, int kind, void *p) {
    handle_t *h = (handle_t *)malloc(sizeof(handle_t));
    h->kind = kind;
    h->p = p;
    napi_value out;
    if (napi_create_external(env, h, handle_finalize, NULL, &out) != napi_ok) {
        handle_finalize(env, h, NULL);
        napi_throw_error(env, NULL, "napi_create_external failed");
        return NULL;
    }
    return out;
}

static handle_t *get_handle(napi_env env, napi_value v, int kind) {
    void *data = NULL;
    if (napi_get_value_external(env, v, &data) != napi_ok || !data ||
        ((handle_t *)data)->kind != kind) {
        napi_throw_type_error(env, NULL, "invalid ringpop_amd handle");
        return NULL;
    }
    if (!((handle_t *)data)->p) {
        napi_throw_error(env, NULL, "ringpop_amd handle already destroyed");
        return NULL;
    }
    return (handle_t *)data;
}

/* A JS array of strings packed as bytes + offsets (off32 or off64 chosen by the caller). */
typedef struct {
    char *bytes;
    uint32_t *off32;
    uint64_t *off64;
    uint32_t n;
} strpack_t;

static void strpack_free(strpack_t *s) {
    free(s->bytes);
    free(s->off32);
    free(s->off64);
    memset(s, 0, sizeof(*s));
}

/* Returns 0 and fills *s, or -1 with a pending JS exception. Non-strings are coerced with
 * String(x), as the reference's hashFunc(str) would (farmhash takes its argument's string). */
static int strpack_from_array(napi_env env, napi_value arr, strpack_t *s) {
    memset(s, 0, sizeof(*s));
    if (is_nullish(env, arr)) return 0;
    bool isarr = false;
    napi_is_array(env, arr, &isarr);
    if (!isarr) {
        napi_throw_type_error(env, NULL, "expected an array of strings");
        return -1;
    }
    uint32_t n = 0;
    napi_get_array_length(env, arr, &n);
    s->n = n;
    s->off32 = (uint32_t *)malloc(sizeof(uint32_t) * (n + 1));
    s->off64 = (uint64_t *)malloc(sizeof(uint64_t) * (n + 1));
    size_t cap = 64 + (size_t)n * 40, used = 0;
    s->bytes = (char *)malloc(cap);
    for (uint32_t i = 0; i < n; i++) {
        napi_value e, str;
        napi_get_element(env, arr, i, &e);
        if (napi_coerce_to_string(env, e, &str) != napi_ok) {
            strpack_free(s);
            napi_throw_type_error(env, NULL, "array element is not coercible to string");
            return -1;
        }
        size_t len = 0;
        napi_get_value_string_utf8(env, str, NULL, 0, &len);
        if (used + len + 1 > cap) {
            while (used + len + 1 > cap) cap *= 2;
            s->bytes = (char *)realloc(s->bytes, cap);
        }
        size_t got = 0;
        napi_get_value_string_utf8(env, str, s->bytes + used, len + 1, &got);
        s->off32[i] = (uint32_t)used;
        s->off64[i] = used;
        used += got;
    }
    s->off32[n] = (uint32_t)used;
    s->off64[n] = used;
    return 0;
}

/* Typed-array view of the wanted element type: 0 with data/len, or -1 (data NULL, len 0)
 * when v is not such a typed array. Zero-length arrays may have data == NULL. */
static int typed_get(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
    bool is = false;
    *data = NULL;
    *len = 0;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return -1;
    napi_typedarray_type t;
    napi_value ab;
    size_t boff = 0;
    napi_get_typedarray_info(env, v, &t, len, data, &ab, &boff);
    if (t != want) {
        *data = NULL;
        *len = 0;
        return -1;
    }
    return 0;
}

static void *typed_data(napi_env env, napi_value v, napi_typedarray_type want, size_t *len) {
    void *d = NULL;
    typed_get(env, v, want, &d, len);
    return d;
}

static napi_value new_typed(napi_env env, napi_typedarray_type t, size_t n, size_t elem, void **data) {
    napi_value ab, out;
    if (napi_create_arraybuffer(env, n * elem, data, &ab) != napi_ok) return NULL;
    if (napi_create_typedarray(env, t, n, ab, 0, &out) != napi_ok) return NULL;
    return out;
}

static napi_value ring_name(napi_env env, rp_ring *r, uint32_t id) {
    if (id == RP_NULL_ID) return make_null(env);
    uint32_t len = 0;
    const char *p = rp_ring_owner_name(r, id, &len);
    if (!p) return make_null(env);
    napi_value s;
    napi_create_string_utf8(env, p, len, &s);
    return s;
}

/* ------------------------------------------------------------------ common */
static napi_value js_version(napi_env env, napi_callback_info info) {
    (void)info;
    return make_u32(env, rp_version());
}

static napi_value js_device_count(napi_env env, napi_callback_info info) {
    (void)info;
    int n = 0;
    RP_OK(rp_device_count(&n));
    return make_u32(env, (uint32_t)n);
}

/* farmhash.hash32(str) (reference package.json:34): host C++ farmhashmk::Hash32 of the UTF-8
 * bytes, the same code librpamd's kernels run. */
static napi_value js_hash32(napi_env env, napi_callback_info info) {
    ARGS(1);
    napi_value str;
    NAPI_OK(napi_coerce_to_string(env, argv[0], &str));
    size_t len = 0;
    NAPI_OK(napi_get_value_string_utf8(env, str, NULL, 0, &len));
    char stackbuf[256];
    char *buf = len < sizeof(stackbuf) ? stackbuf : (char *)malloc(len + 1);
    napi_get_value_string_utf8(env, str, buf, len + 1, &len);
    uint32_t h = rp_hash32(buf, len);
    if (buf != stackbuf) free(buf);
    return make_u32(env, h);
}

/* ------------------------------------------------------------------ ring */
static napi_value js_ring_create(napi_env env, napi_callback_info info) {
    ARGS(2);
    uint32_t rp = 0;
    int32_t dev = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[0], &rp));
    NAPI_OK(napi_get_value_int32(env, argv[1], &dev));
    rp_ring *r = NULL;
    RP_OK(rp_ring_create(rp, dev, &r));
    return wrap_handle(env, 1, r);
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    void *data = NULL;
    NAPI_OK(napi_get_value_external(env, argv[0], &data));
    handle_t *h = (handle_t *)data;
    if (h && h->p) {
        if (h->kind == 1) rp_ring_destroy((rp_ring *)h->p);
        if (h->kind == 2) rp_members_destroy((rp_members *)h->p);
        if (h->kind == 3) rp_sim_destroy((rp_sim *)h->p);
        if (h->kind == 4) rp_ring_snap_destroy((rp_ring_snap *)h->p);
        h->p = NULL;
    }
    return NULL;
}

/* addRemoveServers(add[], remove[], addTokens?, removeTokens?) -> ringChanged
 * (lib/ring/index.js:60-94). Token arrays (Uint32Array, n*replicaPoints) carry a caller
 * hashFunc's replica hashes (options.hashFunc, :29). */
static napi_value js_ring_add_remove(napi_env env, napi_callback_info info) {
    ARGS(5);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    strpack_t add, rem;
    if (strpack_from_array(env, argv[1], &add)) return NULL;
    if (strpack_from_array(env, argv[2], &rem)) {
        strpack_free(&add);
        return NULL;
    }
    size_t n1 = 0, n2 = 0;
    const uint32_t *at = is_nullish(env, argv[3]) ? NULL : (const uint32_t *)typed_data(env, argv[3], napi_uint32_array, &n1);
    const uint32_t *rt = is_nullish(env, argv[4]) ? NULL : (const uint32_t *)typed_data(env, argv[4], napi_uint32_array, &n2);
    int changed = 0;
    int rc = rp_ring_add_remove((rp_ring *)h->p, add.bytes, add.off32, add.n, at, rem.bytes, rem.off32, rem.n, rt,
                                &changed);
    strpack_free(&add);
    strpack_free(&rem);
    RP_OK(rc);
    return make_bool(env, changed);
}

static napi_value js_ring_checksum(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint32_t v = 0;
    int set = 0;
    RP_OK(rp_ring_checksum((rp_ring *)h->p, &v, &set));
    return set ? make_u32(env, v) : make_null(env);
}

static napi_value js_ring_checksum_string(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint64_t len = 0;
    RP_OK(rp_ring_checksum_string((rp_ring *)h->p, NULL, 0, &len));
    char *buf = (char *)malloc(len + 1);
    int rc = rp_ring_checksum_string((rp_ring *)h->p, buf, len, &len);
    if (rc) {
        free(buf);
        RP_OK(rc);
    }
    napi_value s;
    napi_create_string_utf8(env, buf, len, &s);
    free(buf);
    return s;
}

static napi_value js_ring_server_count(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint32_t n = 0;
    RP_OK(rp_ring_server_count((rp_ring *)h->p, &n));
    return make_u32(env, n);
}

static napi_value js_ring_service(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint32_t idle = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &idle));
    RP_OK(rp_ring_service((rp_ring *)h->p, idle));
    return make_u32(env, idle);
}

static napi_value js_ring_token_count(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint32_t n = 0;
    RP_OK(rp_ring_token_count((rp_ring *)h->p, &n));
    return make_u32(env, n);
}

static napi_value js_ring_has_server(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    napi_value str;
    NAPI_OK(napi_coerce_to_string(env, argv[1], &str));
    size_t len = 0;
    napi_get_value_string_utf8(env, str, NULL, 0, &len);
    char *buf = (char *)malloc(len + 1);
    napi_get_value_string_utf8(env, str, buf, len + 1, &len);
    int has = 0;
    int rc = rp_ring_has_server((rp_ring *)h->p, buf, (uint32_t)len, &has);
    free(buf);
    RP_OK(rc);
    return make_bool(env, has);
}

/* Object.keys(servers) in insertion order (getStats, lib/ring/index.js:111-116). */
static napi_value js_ring_servers(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    uint32_t n = 0;
    RP_OK(rp_ring_servers(r, NULL, 0, &n));
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    int rc = rp_ring_servers(r, ids, n, &n);
    if (rc) {
        free(ids);
        RP_OK(rc);
    }
    napi_value arr;
    napi_create_array_with_length(env, n, &arr);
    for (uint32_t i = 0; i < n; i++) napi_set_element(env, arr, i, ring_name(env, r, ids[i]));
    free(ids);
    return arr;
}

static napi_value js_ring_owner_name(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    uint32_t id = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &id));
    return ring_name(env, (rp_ring *)h->p, id);
}

/* lookupBatch(h, keys[]) -> names (null for an empty ring), lookup() of every key
 * (lib/ring/index.js:145-154), one device launch. */
static napi_value js_ring_lookup(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    strpack_t keys;
    if (strpack_from_array(env, argv[1], &keys)) return NULL;
    uint32_t *own = (uint32_t *)malloc(sizeof(uint32_t) * (keys.n ? keys.n : 1));
    int rc = rp_ring_lookup(r, keys.bytes, keys.off64, 0, keys.n, own);
    uint32_t n = keys.n;
    strpack_free(&keys);
    if (rc) {
        free(own);
        RP_OK(rc);
    }
    napi_value arr;
    napi_create_array_with_length(env, n, &arr);
    for (uint32_t i = 0; i < n; i++) napi_set_element(env, arr, i, ring_name(env, r, own[i]));
    free(own);
    return arr;
}

/* lookup1(h, key) -> name | null and lookupN1(h, key, n) -> [names]: one key, no arrays in
 * between (RingPop.lookup / lookupN per request, index.js:434-471; the ring service, when on,
 * answers them without a launch). */
static int key_utf8(napi_env env, napi_value v, char *stack, size_t cap, char **out, size_t *len) {
    napi_value str;
    if (napi_coerce_to_string(env, v, &str) != napi_ok) {
        napi_throw_type_error(env, NULL, "key is not coercible to string");
        return -1;
    }
    napi_get_value_string_utf8(env, str, NULL, 0, len);
    *out = *len < cap ? stack : (char *)malloc(*len + 1);
    size_t got = 0;
    napi_get_value_string_utf8(env, str, *out, *len + 1, &got);
    *len = got;
    return 0;
}

static napi_value js_ring_lookup1(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    char stack[256], *k = NULL;
    size_t len = 0;
    if (key_utf8(env, argv[1], stack, sizeof stack, &k, &len)) return NULL;
    uint64_t off[2] = {0, len};
    uint32_t own = RP_NULL_ID;
    int rc = rp_ring_lookup(r, k, off, 0, 1, &own);
    if (k != stack) free(k);
    RP_OK(rc);
    return ring_name(env, r, own);
}

static napi_value js_ring_lookupn1(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[2], &nrep));
    char stack[256], *k = NULL;
    size_t len = 0;
    if (key_utf8(env, argv[1], stack, sizeof stack, &k, &len)) return NULL;
    const uint32_t W = nrep > 1 ? (uint32_t)nrep : 1u;
    uint32_t own_s[16], *own = W <= 16 ? own_s : (uint32_t *)malloc(4ull * W);
    uint8_t cnt = 0;
    uint64_t off[2] = {0, len};
    int rc = rp_ring_lookupn(r, k, off, 0, 1, nrep, own, &cnt);
    if (k != stack) free(k);
    if (rc) {
        if (own != own_s) free(own);
        RP_OK(rc);
    }
    napi_value arr;
    napi_create_array_with_length(env, cnt, &arr);
    for (uint32_t j = 0; j < cnt; j++) napi_set_element(env, arr, j, ring_name(env, r, own[j]));
    if (own != own_s) free(own);
    return arr;
}

/* groupKeys(h, keys[] | Uint32Array hashes) -> {dests: [name|null], groupOff: Uint32Array,
 * perm: Uint32Array}: handleOrProxyAll's _.groupBy(keys, lookup) (index.js:609-667, :616) and
 * lookupKeys (lib/request-proxy/send.js:171-179) on the device. A null dest = the empty ring's
 * null owner (the caller substitutes whoami(), index.js:434-451). */
static napi_value js_ring_group_keys(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    bool is_typed = false;
    napi_is_typedarray(env, argv[1], &is_typed);
    size_t n = 0;
    void *hv = NULL;
    strpack_t keys;
    memset(&keys, 0, sizeof(keys));
    if (is_typed) {
        if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
            napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
            return NULL;
        }
    } else {
        if (strpack_from_array(env, argv[1], &keys)) return NULL;
        n = keys.n;
    }
    size_t nn = n ? n : 1;
    uint32_t *dests = (uint32_t *)malloc(sizeof(uint32_t) * nn);
    void *gd = NULL, *pd = NULL;
    napi_value goff = new_typed(env, napi_uint32_array, nn + 1, 4, &gd);
    napi_value perm = new_typed(env, napi_uint32_array, n, 4, &pd);
    uint32_t nd = 0;
    uint32_t pdummy = 0;
    int rc = is_typed ? rp_ring_group_hashes(r, (const uint32_t *)hv, n, RP_NULL_ID, dests, (uint32_t *)gd,
                                             n ? (uint32_t *)pd : &pdummy, &nd)
                      : rp_ring_group_keys(r, keys.bytes, keys.off64, 0, n, RP_NULL_ID, dests, (uint32_t *)gd,
                                           n ? (uint32_t *)pd : &pdummy, &nd);
    if (!is_typed) strpack_free(&keys);
    if (rc) {
        free(dests);
        RP_OK(rc);
    }
    napi_value arr, out;
    napi_create_array_with_length(env, nd, &arr);
    for (uint32_t i = 0; i < nd; i++) napi_set_element(env, arr, i, ring_name(env, r, dests[i]));
    free(dests);
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "dests", arr);
    napi_set_named_property(env, out, "groupOff", goff);
    napi_set_named_property(env, out, "perm", perm);
    return out;
}

/* ringSnapshot(h) -> snapshot handle (rp_ring_snapshot): an immutable device copy of the ring as
 * it is now; destroy(handle) frees it (twice is harmless), as does garbage collection. */
static napi_value js_ring_snapshot(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring_snap *s = NULL;
    RP_OK(rp_ring_snapshot((rp_ring *)h->p, &s));
    return wrap_handle(env, 4, s);
}

/* ringSnapInfo(snap) -> {tokens, servers, checksum | null} as of the snapshot. */
static napi_value js_ring_snap_info(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 4);
    if (!h) return NULL;
    uint32_t m = 0, sc = 0, ck = 0;
    int set = 0;
    RP_OK(rp_ring_snap_info((const rp_ring_snap *)h->p, &m, &sc, &ck, &set));
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "tokens", make_u32(env, m));
    napi_set_named_property(env, out, "servers", make_u32(env, sc));
    napi_set_named_property(env, out, "checksum", set ? make_u32(env, ck) : make_null(env));
    return out;
}

/* ringMovedKeys(h, keys[] | Uint32Array hashes, snap, n) -> {count, idx: Uint32Array,
 * before: Uint32Array, after: Uint32Array}: the keys whose lookupN(key, n) row differs between
 * the snapshot and the ring now (rp_ring_moved_keys / _hashes), ascending key indices and the
 * two rows of max(n,1) owner ids each (0xFFFFFFFF = none). */
static napi_value js_ring_moved_keys(napi_env env, napi_callback_info info) {
    ARGS(4);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    handle_t *sh = get_handle(env, argv[2], 4);
    if (!sh) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    const rp_ring_snap *snap = (const rp_ring_snap *)sh->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[3], &nrep));
    bool is_typed = false;
    napi_is_typedarray(env, argv[1], &is_typed);
    size_t n = 0;
    void *hv = NULL;
    strpack_t keys;
    memset(&keys, 0, sizeof(keys));
    if (is_typed) {
        if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
            napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
            return NULL;
        }
    } else {
        if (strpack_from_array(env, argv[1], &keys)) return NULL;
        n = keys.n;
    }
    const size_t w = nrep > 1 ? (size_t)nrep : 1u, nn = n ? n : 1;
    uint32_t *idx = (uint32_t *)malloc(4 * nn), *br = (uint32_t *)malloc(4 * nn * w),
             *ar = (uint32_t *)malloc(4 * nn * w);
    uint32_t count = 0;
    int rc = is_typed ? rp_ring_moved_hashes(r, snap, (const uint32_t *)hv, n, nrep, (uint32_t)n, idx, br, ar, &count)
                      : rp_ring_moved_keys(r, snap, keys.bytes, keys.off64, 0, n, nrep, (uint32_t)n, idx, br, ar,
                                           &count);
    if (!is_typed) strpack_free(&keys);
    napi_value out = NULL;
    if (!rc) {
        void *di = NULL, *db = NULL, *da = NULL;
        napi_value vi = new_typed(env, napi_uint32_array, count, 4, &di);
        napi_value vb = new_typed(env, napi_uint32_array, count * w, 4, &db);
        napi_value va = new_typed(env, napi_uint32_array, count * w, 4, &da);
        if (count) {
            memcpy(di, idx, 4 * (size_t)count);
            memcpy(db, br, 4 * (size_t)count * w);
            memcpy(da, ar, 4 * (size_t)count * w);
        }
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "count", make_u32(env, count));
        napi_set_named_property(env, out, "idx", vi);
        napi_set_named_property(env, out, "before", vb);
        napi_set_named_property(env, out, "after", va);
    }
    free(idx);
    free(br);
    free(ar);
    RP_OK(rc);
    return out;
}

/* ringHandoff(h, keys[] | Uint32Array hashes, snap, n, whoami | null) -> {count, dests, groupOff,
 * keyIdx, src: Uint32Array, slot: Uint8Array}: the transfers that bring every key's lookupN(key, n)
 * row up to date from its row under the snapshot, grouped by destination id (ascending)
 * (rp_ring_handoff / _hashes). whoami (a server name): only what that server has to send; a name
 * the ring never saw sends nothing. */
static napi_value js_ring_handoff(napi_env env, napi_callback_info info) {
    ARGS(5);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    handle_t *sh = get_handle(env, argv[2], 4);
    if (!sh) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    const rp_ring_snap *snap = (const rp_ring_snap *)sh->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[3], &nrep));
    uint32_t only = RP_NULL_ID;
    bool nobody = false;
    napi_valuetype wt;
    NAPI_OK(napi_typeof(env, argv[4], &wt));
    if (wt != napi_undefined && wt != napi_null) {
        napi_value str;
        NAPI_OK(napi_coerce_to_string(env, argv[4], &str));
        size_t len = 0;
        napi_get_value_string_utf8(env, str, NULL, 0, &len);
        char *buf = (char *)malloc(len + 1);
        napi_get_value_string_utf8(env, str, buf, len + 1, &len);
        int rc = rp_ring_server_id(r, buf, (uint32_t)len, &only);
        free(buf);
        RP_OK(rc);
        nobody = only == RP_NULL_ID;
    }
    uint32_t bound = 0;
    RP_OK(rp_ring_id_bound(r, &bound));
    bool is_typed = false;
    napi_is_typedarray(env, argv[1], &is_typed);
    size_t n = 0;
    void *hv = NULL;
    strpack_t keys;
    memset(&keys, 0, sizeof(keys));
    if (is_typed) {
        if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
            napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
            return NULL;
        }
    } else {
        if (strpack_from_array(env, argv[1], &keys)) return NULL;
        n = keys.n;
    }
    if (nobody) n = 0;
    const size_t w = nrep > 1 ? (size_t)nrep : 1u;
    const size_t cap = n * w < 0xFFFFFFFFu ? n * w : 0xFFFFFFFFu, c1 = cap ? cap : 1;
    const size_t nd = cap < bound ? cap : bound;
    uint32_t *dests = (uint32_t *)malloc(4 * (nd + 1)), *goff = (uint32_t *)malloc(4 * (nd + 1)),
             *kidx = (uint32_t *)malloc(4 * c1), *src = (uint32_t *)malloc(4 * c1);
    uint8_t *slot = (uint8_t *)malloc(c1);
    uint32_t count = 0, ndest = 0;
    int rc = is_typed ? rp_ring_handoff_hashes(r, snap, (const uint32_t *)hv, n, nrep, only, (uint32_t)cap, dests, goff,
                                               kidx, src, slot, &ndest, &count)
                      : rp_ring_handoff(r, snap, keys.bytes, keys.off64, 0, n, nrep, only, (uint32_t)cap, dests, goff,
                                        kidx, src, slot, &ndest, &count);
    if (!is_typed) strpack_free(&keys);
    napi_value out = NULL;
    if (!rc) {
        void *dd = NULL, *dg = NULL, *dk = NULL, *ds = NULL, *dq = NULL;
        napi_value vd = new_typed(env, napi_uint32_array, ndest, 4, &dd);
        napi_value vg = new_typed(env, napi_uint32_array, (size_t)ndest + 1, 4, &dg);
        napi_value vk = new_typed(env, napi_uint32_array, count, 4, &dk);
        napi_value vs = new_typed(env, napi_uint32_array, count, 4, &ds);
        napi_value vq = new_typed(env, napi_uint8_array, count, 1, &dq);
        if (ndest) memcpy(dd, dests, 4 * (size_t)ndest);
        memcpy(dg, goff, 4 * ((size_t)ndest + 1));
        if (count) {
            memcpy(dk, kidx, 4 * (size_t)count);
            memcpy(ds, src, 4 * (size_t)count);
            memcpy(dq, slot, (size_t)count);
        }
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "count", make_u32(env, count));
        napi_set_named_property(env, out, "dests", vd);
        napi_set_named_property(env, out, "groupOff", vg);
        napi_set_named_property(env, out, "keyIdx", vk);
        napi_set_named_property(env, out, "src", vs);
        napi_set_named_property(env, out, "slot", vq);
    }
    free(dests);
    free(goff);
    free(kidx);
    free(src);
    free(slot);
    RP_OK(rc);
    return out;
}

/* One row of rp_ring_route_views' byte matrix from a JS array of server names: row[id] = 1 for the
 * names the ring has interned (others are ignored). 0, or -1 with a pending JS exception. */
static int route_row(napi_env env, rp_ring *r, napi_value names, uint8_t *row, uint32_t bound) {
    strpack_t s;
    if (strpack_from_array(env, names, &s)) return -1;
    memset(row, 0, bound ? bound : 1);
    int rc = 0;
    for (uint32_t i = 0; i < s.n && !rc; i++) {
        uint32_t id = RP_NULL_ID;
        rc = rp_ring_server_id(r, s.bytes + s.off64[i], (uint32_t)(s.off64[i + 1] - s.off64[i]), &id);
        if (!rc && id < bound) row[id] = 1;
    }
    strpack_free(&s);
    if (rc) {
        napi_throw_error(env, "ERR_RINGPOP_AMD", rp_last_error());
        return -1;
    }
    return 0;
}

/* The byte matrix of views (an array of arrays of server names) and the truth's row (names, or
 * nullish: NULL) by server id, with the ring's id bound; the row stride is max(bound, 1). The
 * caller frees *rows and *truth. 0, or -1 with a pending JS exception and nothing to free. */
static int route_rows(napi_env env, rp_ring *r, napi_value views, napi_value tnames, uint32_t *bound, uint32_t *nv,
                      uint8_t **rows, uint8_t **truth) {
    *rows = *truth = NULL;
    if (rp_ring_id_bound(r, bound)) {
        napi_throw_error(env, "ERR_RINGPOP_AMD", rp_last_error());
        return -1;
    }
    bool isarr = false;
    napi_is_array(env, views, &isarr);
    if (!isarr) {
        napi_throw_type_error(env, NULL, "views must be an array of arrays of server names");
        return -1;
    }
    napi_get_array_length(env, views, nv);
    const size_t rs = *bound ? *bound : 1;
    *rows = (uint8_t *)calloc((size_t)(*nv ? *nv : 1) * rs, 1);
    if (!is_nullish(env, tnames)) *truth = (uint8_t *)calloc(rs, 1);
    int bad = *truth ? route_row(env, r, tnames, *truth, *bound) : 0;
    for (uint32_t v = 0; v < *nv && !bad; v++) {
        napi_value e;
        napi_get_element(env, views, v, &e);
        bad = route_row(env, r, e, *rows + (size_t)v * rs, *bound);
    }
    if (bad) {
        free(*rows);
        free(*truth);
        *rows = *truth = NULL;
        return -1;
    }
    return 0;
}

/* ringRouteViews(h, keys[] | Uint32Array hashes, views: [[server names]], truth: [names] | null) ->
 * {views, wrong, lost: Float64Array[views], keyWrong, truthOwner: Uint32Array[keys],
 * owners: Uint32Array[keys * views]}: every key's owner under every view of this ring at once
 * (rp_ring_route_views; 0xFFFFFFFF = none). Counts are Numbers: exact below 2^53. */
static napi_value js_ring_route_views(napi_env env, napi_callback_info info) {
    ARGS(4);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    uint32_t bound = 0, nv = 0;
    uint8_t *rows = NULL, *truth = NULL;
    if (route_rows(env, r, argv[2], argv[3], &bound, &nv, &rows, &truth)) return NULL;
    const size_t rs = bound ? bound : 1;
    bool is_typed = false;
    napi_is_typedarray(env, argv[1], &is_typed);
    size_t n = 0;
    void *hv = NULL;
    strpack_t keys;
    memset(&keys, 0, sizeof(keys));
    if (is_typed) {
        if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
            free(rows);
            free(truth);
            napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
            return NULL;
        }
    } else {
        if (strpack_from_array(env, argv[1], &keys)) {
            free(rows);
            free(truth);
            return NULL;
        }
        n = keys.n;
    }
    const size_t nn = n ? n : 1, vv = nv ? nv : 1;
    uint64_t *wrong = (uint64_t *)calloc(2 * vv, 8), *lost = wrong + vv;
    uint32_t *kw = (uint32_t *)calloc(2 * nn + nn * vv, 4), *to = kw + nn, *ow = to + nn;
    int rc = rp_ring_route_views(r, is_typed ? NULL : keys.bytes, is_typed ? NULL : keys.off64, 0,
                                 is_typed ? (const uint32_t *)hv : NULL, n, rows, rs, 1, nv, NULL, bound, truth, NULL,
                                 0, wrong, lost, kw, to, ow);
    if (!is_typed) strpack_free(&keys);
    napi_value out = NULL;
    if (!rc) {
        void *dw = NULL, *dl = NULL, *dk = NULL, *dt = NULL, *dow = NULL;
        napi_value vw = new_typed(env, napi_float64_array, nv, 8, &dw);
        napi_value vl = new_typed(env, napi_float64_array, nv, 8, &dl);
        napi_value vk = new_typed(env, napi_uint32_array, n, 4, &dk);
        napi_value vt = new_typed(env, napi_uint32_array, n, 4, &dt);
        napi_value vo = new_typed(env, napi_uint32_array, n * nv, 4, &dow);
        for (uint32_t v = 0; v < nv; v++) {
            ((double *)dw)[v] = (double)wrong[v];
            ((double *)dl)[v] = (double)lost[v];
        }
        if (n) {
            memcpy(dk, kw, 4 * n);
            memcpy(dt, to, 4 * n);
            if (nv) memcpy(dow, ow, 4 * n * nv);
        }
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "views", make_u32(env, nv));
        napi_set_named_property(env, out, "wrong", vw);
        napi_set_named_property(env, out, "lost", vl);
        napi_set_named_property(env, out, "keyWrong", vk);
        napi_set_named_property(env, out, "truthOwner", vt);
        napi_set_named_property(env, out, "owners", vo);
    }
    free(rows);
    free(truth);
    free(wrong);
    free(kw);
    RP_OK(rc);
    return out;
}

/* ringRouteShare(h, views: [[server names]], truth: [names] | null) -> {wrong, lost:
 * Float64Array[views], posWrong: Uint32Array[tokens], disputed}: on how many of the 2^32 hash
 * values every view disagrees with the truth, per token position how many views do
 * (rp_ring_route_share), and the hash values on which at least one does (the interval lengths of
 * rp_ring_dump's tokens where posWrong > 0). The shares are Numbers: at most 2^32, exact in a
 * double. */
static napi_value js_ring_route_share(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    uint32_t bound = 0, nv = 0, m = 0;
    RP_OK(rp_ring_token_count(r, &m));
    uint8_t *rows = NULL, *truth = NULL;
    if (route_rows(env, r, argv[1], argv[2], &bound, &nv, &rows, &truth)) return NULL;
    const size_t vv = nv ? nv : 1;
    uint64_t *wrong = (uint64_t *)calloc(2 * vv, 8), *lost = wrong + vv;
    uint32_t *pw = (uint32_t *)calloc(3 * (size_t)(m ? m : 1), 4), *tok = pw + (m ? m : 1), *own = tok + (m ? m : 1);
    int rc = rp_ring_route_share(r, rows, bound ? bound : 1, 1, nv, NULL, bound, truth, NULL, 0, wrong, lost, pw, m);
    if (!rc) rc = rp_ring_dump(r, tok, own, m);
    napi_value out = NULL;
    if (!rc) {
        uint64_t disputed = 0;
        for (uint32_t i = 0; i < m; i++)
            if (pw[i]) disputed += i ? (uint64_t)tok[i] - tok[i - 1] : (uint64_t)tok[0] + (1ull << 32) - tok[m - 1];
        void *dw = NULL, *dl = NULL, *dp = NULL;
        napi_value vw = new_typed(env, napi_float64_array, nv, 8, &dw);
        napi_value vl = new_typed(env, napi_float64_array, nv, 8, &dl);
        napi_value vp = new_typed(env, napi_uint32_array, m, 4, &dp);
        for (uint32_t v = 0; v < nv; v++) {
            ((double *)dw)[v] = (double)wrong[v];
            ((double *)dl)[v] = (double)lost[v];
        }
        if (m) memcpy(dp, pw, 4 * (size_t)m);
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "wrong", vw);
        napi_set_named_property(env, out, "lost", vl);
        napi_set_named_property(env, out, "posWrong", vp);
        napi_value vd;
        napi_create_double(env, (double)disputed, &vd);
        napi_set_named_property(env, out, "disputed", vd);
    }
    free(rows);
    free(truth);
    free(wrong);
    free(pw);
    RP_OK(rc);
    return out;
}

/* The servers now in the ring (rp_ring_servers order) as {names: [..], counts: Float64Array}:
 * counts[i * w + q] = table[ids[i] * w + q]. Counts are Numbers: exact below 2^53. */
static napi_value ring_named_counts(napi_env env, rp_ring *r, const uint64_t *table, size_t w) {
    uint32_t n = 0;
    RP_OK(rp_ring_servers(r, NULL, 0, &n));
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    if (!ids) {
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    int rc = rp_ring_servers(r, ids, n, &n);
    if (rc) {
        free(ids);
        RP_OK(rc);
    }
    napi_value out, names;
    void *dc = NULL;
    napi_value counts = new_typed(env, napi_float64_array, (size_t)n * w, 8, &dc);
    if (!counts || (!dc && n)) {
        free(ids);
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    napi_create_array_with_length(env, n, &names);
    for (uint32_t i = 0; i < n; i++) {
        napi_set_element(env, names, i, ring_name(env, r, ids[i]));
        for (size_t q = 0; q < w; q++) ((double *)dc)[i * w + q] = (double)table[(size_t)ids[i] * w + q];
    }
    free(ids);
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "names", names);
    napi_set_named_property(env, out, "counts", counts);
    return out;
}

/* ringOwnerLoad(h, keys[] | Uint32Array hashes, n) -> {names, counts: Float64Array}: for each
 * server now in the ring, how many keys have it in slot q of their lookupN(key, n) row
 * (rp_ring_owner_load / _hashes), max(n,1) counts a server. */
static napi_value js_ring_owner_load(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[2], &nrep));
    bool is_typed = false;
    napi_is_typedarray(env, argv[1], &is_typed);
    size_t n = 0;
    void *hv = NULL;
    strpack_t keys;
    memset(&keys, 0, sizeof(keys));
    if (is_typed) {
        if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
            napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
            return NULL;
        }
    } else {
        if (strpack_from_array(env, argv[1], &keys)) return NULL;
        n = keys.n;
    }
    const size_t w = nrep > 1 ? (size_t)nrep : 1u;
    uint32_t cap = 0;
    int rc = rp_ring_id_bound(r, &cap);
    uint64_t *load = rc ? NULL : (uint64_t *)calloc((size_t)cap * w + 1, 8);
    if (!rc && !load) {
        if (!is_typed) strpack_free(&keys);
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    if (!rc)
        rc = is_typed ? rp_ring_owner_load_hashes(r, (const uint32_t *)hv, n, nrep, cap, load)
                      : rp_ring_owner_load(r, keys.bytes, keys.off64, 0, n, nrep, cap, load);
    if (!is_typed) strpack_free(&keys);
    napi_value out = rc ? NULL : ring_named_counts(env, r, load, w);
    free(load);
    RP_OK(rc);
    return out;
}

/* ringOwnerShare(h) -> {names, counts: Float64Array}: how many of the 2^32 hash values each
 * server now in the ring owns (rp_ring_owner_share). */
static napi_value js_ring_owner_share(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    uint32_t cap = 0;
    int rc = rp_ring_id_bound(r, &cap);
    uint64_t *share = rc ? NULL : (uint64_t *)calloc((size_t)cap + 1, 8);
    if (!rc && !share) {
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    if (!rc) rc = rp_ring_owner_share(r, cap, share);
    napi_value out = rc ? NULL : ring_named_counts(env, r, share, 1);
    free(share);
    RP_OK(rc);
    return out;
}

/* ringMovedRanges(h, snap, n) -> {count, movedHashes, lo, hi, before, after}: the hash intervals
 * [lo, hi] (inclusive, ascending) on which the lookupN(h, n) row under the snapshot differs from
 * the row now (rp_ring_moved_ranges), with the two rows of max(n,1) owner ids each (0xFFFFFFFF =
 * none). movedHashes is a Number: exact, it is at most 2^32. */
static napi_value js_ring_moved_ranges(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    handle_t *sh = get_handle(env, argv[1], 4);
    if (!sh) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    const rp_ring_snap *snap = (const rp_ring_snap *)sh->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[2], &nrep));
    uint32_t tb = 0, ta = 0;
    RP_OK(rp_ring_snap_info(snap, &tb, NULL, NULL, NULL));
    RP_OK(rp_ring_token_count(r, &ta));
    const size_t w = nrep > 1 ? (size_t)nrep : 1u, cap = (size_t)tb + ta + 1; /* holds every run */
    uint32_t *lo = (uint32_t *)malloc(4 * cap), *hi = (uint32_t *)malloc(4 * cap),
             *br = (uint32_t *)malloc(4 * cap * w), *ar = (uint32_t *)malloc(4 * cap * w);
    uint32_t count = 0;
    uint64_t moved = 0;
    int rc = (lo && hi && br && ar) ? rp_ring_moved_ranges(r, snap, nrep, (uint32_t)cap, lo, hi, br, ar, &count, &moved)
                                    : -2;
    napi_value out = NULL;
    if (!rc) {
        void *dl = NULL, *dh = NULL, *db = NULL, *da = NULL;
        napi_value vl = new_typed(env, napi_uint32_array, count, 4, &dl);
        napi_value vh = new_typed(env, napi_uint32_array, count, 4, &dh);
        napi_value vb = new_typed(env, napi_uint32_array, count * w, 4, &db);
        napi_value va = new_typed(env, napi_uint32_array, count * w, 4, &da);
        if (count) {
            memcpy(dl, lo, 4 * (size_t)count);
            memcpy(dh, hi, 4 * (size_t)count);
            memcpy(db, br, 4 * (size_t)count * w);
            memcpy(da, ar, 4 * (size_t)count * w);
        }
        napi_value vm;
        napi_create_double(env, (double)moved, &vm);
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "count", make_u32(env, count));
        napi_set_named_property(env, out, "movedHashes", vm);
        napi_set_named_property(env, out, "lo", vl);
        napi_set_named_property(env, out, "hi", vh);
        napi_set_named_property(env, out, "before", vb);
        napi_set_named_property(env, out, "after", va);
    }
    free(lo);
    free(hi);
    free(br);
    free(ar);
    if (rc == -2) {
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    RP_OK(rc);
    return out;
}

/* ringSnapDump(snap) -> {tokens: Uint32Array, owners: Uint32Array}: the snapshot's sorted tokens
 * and their owner ids (rp_ring_snap_dump). */
static napi_value js_ring_snap_dump(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 4);
    if (!h) return NULL;
    const rp_ring_snap *snap = (const rp_ring_snap *)h->p;
    uint32_t m = 0;
    RP_OK(rp_ring_snap_info(snap, &m, NULL, NULL, NULL));
    void *dt = NULL, *dw = NULL;
    napi_value vt = new_typed(env, napi_uint32_array, m, 4, &dt);
    napi_value vo = new_typed(env, napi_uint32_array, m, 4, &dw);
    if (m) RP_OK(rp_ring_snap_dump(snap, (uint32_t *)dt, (uint32_t *)dw, m));
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "tokens", vt);
    napi_set_named_property(env, out, "owners", vo);
    return out;
}

/* lookupNBatch(h, keys[], n) -> arrays of names, lookupN() of every key (:157-189). */
static napi_value js_ring_lookupn(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    rp_ring *r = (rp_ring *)h->p;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[2], &nrep));
    strpack_t keys;
    if (strpack_from_array(env, argv[1], &keys)) return NULL;
    uint32_t w = nrep > 1 ? (uint32_t)nrep : 1u;
    uint32_t n = keys.n;
    uint32_t *own = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1) * w);
    uint8_t *cnt = (uint8_t *)malloc(n ? n : 1);
    int rc = rp_ring_lookupn(r, keys.bytes, keys.off64, 0, n, nrep, own, cnt);
    strpack_free(&keys);
    if (rc) {
        free(own);
        free(cnt);
        RP_OK(rc);
    }
    napi_value arr;
    napi_create_array_with_length(env, n, &arr);
    for (uint32_t i = 0; i < n; i++) {
        napi_value row;
        napi_create_array_with_length(env, cnt[i], &row);
        for (uint32_t j = 0; j < cnt[i]; j++)
            napi_set_element(env, row, j, ring_name(env, r, own[(size_t)i * w + j]));
        napi_set_element(env, arr, i, row);
    }
    free(own);
    free(cnt);
    return arr;
}

/* lookupNHashes(h, Uint32Array hashes, n) -> {owners: Uint32Array(ids), counts: Uint8Array}:
 * the id-level batch for callers with their own hashFunc or that keep owner ids. */
static napi_value js_ring_lookupn_hashes(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    size_t n = 0;
    void *hv = NULL;
    if (typed_get(env, argv[1], napi_uint32_array, &hv, &n)) {
        napi_throw_type_error(env, NULL, "hashes must be a Uint32Array");
        return NULL;
    }
    const uint32_t *hs = (const uint32_t *)hv;
    int32_t nrep = 0;
    NAPI_OK(napi_get_value_int32(env, argv[2], &nrep));
    size_t w = nrep > 1 ? (size_t)nrep : 1;
    void *od = NULL, *cd = NULL;
    napi_value owners = new_typed(env, napi_uint32_array, n * w, 4, &od);
    napi_value counts = new_typed(env, napi_uint8_array, n, 1, &cd);
    if (!owners || !counts) {
        napi_throw_error(env, NULL, "allocation failed");
        return NULL;
    }
    if (n) RP_OK(rp_ring_lookupn_hashes((rp_ring *)h->p, hs, n, nrep, (uint32_t *)od, (uint8_t *)cd));
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "owners", owners);
    napi_set_named_property(env, out, "counts", counts);
    return out;
}

/* ------------------------------------------------------------------ membership */
static napi_value js_members_create(napi_env env, napi_callback_info info) {
    ARGS(2);
    uint32_t cap = 0;
    int32_t dev = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[0], &cap));
    NAPI_OK(napi_get_value_int32(env, argv[1], &dev));
    rp_members *m = NULL;
    RP_OK(rp_members_create(cap, dev, &m));
    return wrap_handle(env, 2, m);
}

static napi_value js_members_intern(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    strpack_t s;
    if (strpack_from_array(env, argv[1], &s)) return NULL;
    void *d = NULL;
    napi_value ids = new_typed(env, napi_uint32_array, s.n, 4, &d);
    int rc = s.n ? rp_members_intern((rp_members *)h->p, s.bytes, s.off32, s.n, (uint32_t *)d) : 0;
    strpack_free(&s);
    RP_OK(rc);
    return ids;
}

static napi_value js_members_set_local(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    uint32_t id = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &id));
    RP_OK(rp_members_set_local((rp_members *)h->p, id));
    return NULL;
}

/* update(h, ids Uint32Array, status Uint8Array, inc Float64Array, nowMs) ->
 * {applied: Uint8Array, status: Uint8Array, inc: Float64Array, nApplied} — Membership.update
 * (lib/membership/index.js:249-324) over evaluateUpdate (member.js:71-202). Incarnation
 * numbers are JS Numbers (Date.now() values), exact as doubles. */
static napi_value js_members_update(napi_env env, napi_callback_info info) {
    ARGS(5);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    size_t k = 0, k2 = 0, k3 = 0;
    const uint32_t *ids = (const uint32_t *)typed_data(env, argv[1], napi_uint32_array, &k);
    const uint8_t *st = (const uint8_t *)typed_data(env, argv[2], napi_uint8_array, &k2);
    const double *incd = (const double *)typed_data(env, argv[3], napi_float64_array, &k3);
    if ((k && (!ids || !st || !incd)) || k2 != k || k3 != k) {
        napi_throw_type_error(env, NULL, "update expects Uint32Array ids, Uint8Array status, Float64Array inc of equal length");
        return NULL;
    }
    double now = 0;
    NAPI_OK(napi_get_value_double(env, argv[4], &now));
    int64_t now64 = 0;
    {
        int64_t *t = f64_to_i64(env, &now, 1, 0, "update: now");
        if (!t) return NULL;
        now64 = t[0];
        free(t);
    }
    int64_t *inc = f64_to_i64(env, incd, k, 0, "update: incarnationNumber");
    if (!inc) return NULL;
    void *ad = NULL, *sd = NULL, *id = NULL;
    napi_value applied = new_typed(env, napi_uint8_array, k, 1, &ad);
    napi_value nst = new_typed(env, napi_uint8_array, k, 1, &sd);
    napi_value ninc = new_typed(env, napi_float64_array, k, 8, &id);
    int64_t *ninc64 = (int64_t *)malloc(sizeof(int64_t) * (k ? k : 1));
    uint32_t napplied = 0;
    int rc = k ? rp_members_update((rp_members *)h->p, ids, st, inc, (uint32_t)k, now64, (uint8_t *)ad,
                                   (uint8_t *)sd, ninc64, &napplied)
               : 0;
    for (size_t i = 0; rc == 0 && i < k; i++) ((double *)id)[i] = (double)ninc64[i];
    free(inc);
    free(ninc64);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "applied", applied);
    napi_set_named_property(env, out, "status", nst);
    napi_set_named_property(env, out, "inc", ninc);
    napi_set_named_property(env, out, "nApplied", make_u32(env, napplied));
    return out;
}

/* set(h, ids Uint32Array, status Uint8Array, inc Float64Array) -> Uint32Array of picked stash
 * indices in first-seen order — Membership.set (lib/membership/index.js:208-247) over the stash
 * the JS side kept while !isReady: mergeMembershipChangesets (merge.js:22-51) + set + checksum. */
static napi_value js_members_set(napi_env env, napi_callback_info info) {
    ARGS(4);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    size_t k = 0, k2 = 0, k3 = 0;
    const uint32_t *ids = (const uint32_t *)typed_data(env, argv[1], napi_uint32_array, &k);
    const uint8_t *st = (const uint8_t *)typed_data(env, argv[2], napi_uint8_array, &k2);
    const double *incd = (const double *)typed_data(env, argv[3], napi_float64_array, &k3);
    if ((k && (!ids || !st || !incd)) || k2 != k || k3 != k) {
        napi_throw_type_error(env, NULL, "set expects Uint32Array ids, Uint8Array status, Float64Array inc of equal length");
        return NULL;
    }
    int64_t *inc = f64_to_i64(env, incd, k, 0, "set: incarnationNumber");
    if (!inc) return NULL;
    uint32_t *pick = (uint32_t *)malloc(sizeof(uint32_t) * (k ? k : 1));
    uint32_t np = 0;
    int rc = rp_members_set((rp_members *)h->p, ids, st, inc, (uint32_t)k, pick, &np);
    free(inc);
    if (rc) {
        free(pick);
        RP_OK(rc);
    }
    void *pd = NULL;
    napi_value out = new_typed(env, napi_uint32_array, np, 4, &pd);
    if (np) memcpy(pd, pick, 4ull * np);
    free(pick);
    return out;
}

static napi_value js_members_checksum(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    uint32_t v = 0;
    int set = 0;
    RP_OK(rp_members_checksum((rp_members *)h->p, &v, &set));
    return set ? make_u32(env, v) : make_null(env);
}

static napi_value js_members_compute_checksum(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    RP_OK(rp_members_compute_checksum((rp_members *)h->p));
    return js_members_checksum(env, info);
}

static napi_value js_members_checksum_string(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    uint64_t len = 0;
    RP_OK(rp_members_checksum_string((rp_members *)h->p, NULL, 0, &len));
    char *buf = (char *)malloc(len + 1);
    int rc = rp_members_checksum_string((rp_members *)h->p, buf, len, &len);
    if (rc) {
        free(buf);
        RP_OK(rc);
    }
    napi_value s;
    napi_create_string_utf8(env, buf, len, &s);
    free(buf);
    return s;
}

/* dump(h) -> {exists: Uint8Array, status: Uint8Array, inc: Float64Array} by member id. */
static napi_value js_members_dump(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    rp_members *m = (rp_members *)h->p;
    uint32_t n = 0;
    RP_OK(rp_members_count(m, &n));
    void *ed = NULL, *sd = NULL, *id = NULL;
    napi_value ex = new_typed(env, napi_uint8_array, n, 1, &ed);
    napi_value st = new_typed(env, napi_uint8_array, n, 1, &sd);
    napi_value inc = new_typed(env, napi_float64_array, n, 8, &id);
    int64_t *i64 = (int64_t *)malloc(sizeof(int64_t) * (n ? n : 1));
    int rc = n ? rp_members_dump(m, (uint8_t *)ed, (uint8_t *)sd, i64, n) : 0;
    for (uint32_t i = 0; rc == 0 && i < n; i++) ((double *)id)[i] = (double)i64[i];
    free(i64);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "exists", ex);
    napi_set_named_property(env, out, "status", st);
    napi_set_named_property(env, out, "inc", inc);
    return out;
}

/* ------------------------------------------------------------------ damp scoring
 * Member damp scores on the device (rp_members_damp_*; member.js:45-66,133-153,
 * membership/index.js:330-383), for the drop-in Membership (js/membership.js). */
static double prop_double(napi_env env, napi_value obj, const char *key, double dflt) {
    napi_value v;
    double d = dflt;
    if (is_nullish(env, obj) || napi_get_named_property(env, obj, key, &v) != napi_ok || is_nullish(env, v)) return dflt;
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t == napi_boolean) {
        bool b = false;
        napi_get_value_bool(env, v, &b);
        return b ? 1.0 : 0.0;
    }
    if (napi_get_value_double(env, v, &d) != napi_ok) return dflt;
    return d;
}

/* membersDampConfigure(h, {enabled, initial, min, max, penalty, suppressLimit, halfLife}) with
 * ringpop's defaults (config.js:60-71) for absent keys. */
static napi_value js_members_damp_configure(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    rp_damp_config c;
    c.enabled = prop_double(env, argv[1], "enabled", 1.0) != 0.0;
    c.initial = prop_double(env, argv[1], "initial", 0.0);
    c.min = prop_double(env, argv[1], "min", 0.0);
    c.max = prop_double(env, argv[1], "max", 10000.0);
    c.penalty = prop_double(env, argv[1], "penalty", 500.0);
    c.suppress_limit = prop_double(env, argv[1], "suppressLimit", 5000.0);
    c.half_life = prop_double(env, argv[1], "halfLife", 60.0);
    RP_OK(rp_members_damp_configure((rp_members *)h->p, &c));
    return make_null(env);
}

/* membersDampLast(h, k) -> {score: Float64Array(k), exceeded: Uint8Array(k)}: per change of the
 * last update batch, the member's dampScore after it and whether suppressLimitExceeded fired. */
static napi_value js_members_damp_last(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    uint32_t k = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &k));
    void *sd = NULL, *ed = NULL;
    napi_value sc = new_typed(env, napi_float64_array, k, 8, &sd);
    napi_value ex = new_typed(env, napi_uint8_array, k, 1, &ed);
    RP_OK(k ? rp_members_damp_last((rp_members *)h->p, (double *)sd, (uint8_t *)ed, k) : 0);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "score", sc);
    napi_set_named_property(env, out, "exceeded", ex);
    return out;
}

/* membersDampDecay(h, now): _decayMembersDampScore (index.js:374-383) on the device. */
static napi_value js_members_damp_decay(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    double now = 0;
    NAPI_OK(napi_get_value_double(env, argv[1], &now));
    int64_t *t = f64_to_i64(env, &now, 1, 0, "membersDampDecay: now");
    if (!t) return NULL;
    const int64_t now64 = t[0];
    free(t);
    RP_OK(rp_members_damp_decay((rp_members *)h->p, now64));
    return make_null(env);
}

/* membersDampDump(h) -> {score, last, ts: Float64Array (0 = null)} by member id. */
static napi_value js_members_damp_dump(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    rp_members *m = (rp_members *)h->p;
    uint32_t n = 0;
    RP_OK(rp_members_count(m, &n));
    void *sd = NULL, *ld = NULL, *td = NULL;
    napi_value sc = new_typed(env, napi_float64_array, n, 8, &sd);
    napi_value ls = new_typed(env, napi_float64_array, n, 8, &ld);
    napi_value ts = new_typed(env, napi_float64_array, n, 8, &td);
    int64_t *t64 = (int64_t *)malloc(sizeof(int64_t) * (n ? n : 1));
    int rc = n ? rp_members_damp_dump(m, (double *)sd, (double *)ld, t64, n) : 0;
    for (uint32_t i = 0; rc == 0 && i < n; i++) ((double *)td)[i] = (double)t64[i];
    free(t64);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "score", sc);
    napi_set_named_property(env, out, "last", ls);
    napi_set_named_property(env, out, "ts", ts);
    return out;
}

/* ------------------------------------------------------------------ gossip simulator */
/* simCreate(names[], inc0 Float64Array, dead Uint8Array, seed, suspicionRounds, now0, device) */
// simCreate(names, inc0, dead, seed, suspicionRounds, now0, device[, events Uint32Array of
// (round, kind, node) triples: RP_SIM_KILL / REVIVE / LEAVE / JOIN])
static napi_value js_sim_create(napi_env env, napi_callback_info info) {
    /* (names, inc0, dead, seed, suspicionRounds, now0, device, events[, words per event = 3]) */
    size_t argc = 9;
    napi_value argv[9];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 8) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return NULL;
    }
    uint32_t ew = 3;
    if (argc > 8) napi_get_value_uint32(env, argv[8], &ew);
    strpack_t s;
    if (strpack_from_array(env, argv[0], &s)) return NULL;
    size_t n1 = 0, n2 = 0;
    const double *incd = (const double *)typed_data(env, argv[1], napi_float64_array, &n1);
    const uint8_t *dead = (const uint8_t *)typed_data(env, argv[2], napi_uint8_array, &n2);
    if (!incd || !dead || n1 != s.n || n2 != s.n) {
        strpack_free(&s);
        napi_throw_type_error(env, NULL, "simCreate expects inc0 Float64Array and dead Uint8Array of names.length");
        return NULL;
    }
    uint32_t seed = 0, susp = 0;
    int32_t dev = 0;
    double now0 = 0;
    napi_get_value_uint32(env, argv[3], &seed);
    napi_get_value_uint32(env, argv[4], &susp);
    napi_get_value_double(env, argv[5], &now0);
    napi_get_value_int32(env, argv[6], &dev);
    int64_t *inc = f64_to_i64(env, incd, s.n, 0, "simCreate: inc0");
    int64_t *n0 = inc ? f64_to_i64(env, &now0, 1, 0, "simCreate: now0") : NULL;
    if (!inc || !n0) {
        free(inc);
        strpack_free(&s);
        return NULL;
    }
    const int64_t now64 = n0[0];
    free(n0);
    size_t ne = 0;
    const uint32_t *ev = NULL;
    napi_valuetype et = napi_undefined;
    if (argc > 7) napi_typeof(env, argv[7], &et);
    if (et == napi_object) {
        ev = (const uint32_t *)typed_data(env, argv[7], napi_uint32_array, &ne);
        if (!ev || (ew != 3 && ew != 4) || ne % ew) {
            free(inc);
            strpack_free(&s);
            napi_throw_type_error(env, NULL, "simCreate events must be a Uint32Array of (round, kind, node) triples, "
                                             "or of (round, kind, node, arg) with 4 as the last argument");
            return NULL;
        }
    }
    rp_sim_event *evs = (rp_sim_event *)calloc(ne / ew + 1, sizeof(rp_sim_event));
    for (size_t i = 0; i < ne / ew; i++) {
        evs[i].round = ev[ew * i];
        evs[i].kind = ev[ew * i + 1];
        evs[i].node = ev[ew * i + 2];
        evs[i].reserved = ew == 4 ? ev[ew * i + 3] : 0;
    }
    rp_sim *sim = NULL;
    int rc = rp_sim_create_scenario(s.n, s.bytes, s.off32, inc, dead, seed, susp, now64, dev, NULL, 1, 0, evs,
                                    (uint32_t)(ne / ew), &sim);
    free(evs);
    free(inc);
    strpack_free(&s);
    RP_OK(rc);
    return wrap_handle(env, 3, sim);
}

static napi_value js_sim_step(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t rounds = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &rounds));
    RP_OK(rp_sim_step((rp_sim *)h->p, rounds));
    return NULL;
}

static napi_value js_sim_round(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    int64_t r = 0;
    RP_OK(rp_sim_round((rp_sim *)h->p, &r));
    napi_value out;
    napi_create_double(env, (double)r, &out);
    return out;
}

static napi_value js_sim_checksums(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t n = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &n));
    void *d = NULL;
    napi_value out = new_typed(env, napi_uint32_array, n, 4, &d);
    RP_OK(rp_sim_checksums((rp_sim *)h->p, (uint32_t *)d));
    return out;
}

static napi_value js_sim_view(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t v = 0, n = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &v));
    NAPI_OK(napi_get_value_uint32(env, argv[2], &n));
    void *sd = NULL, *id = NULL;
    napi_value st = new_typed(env, napi_uint8_array, n, 1, &sd);
    napi_value inc = new_typed(env, napi_float64_array, n, 8, &id);
    int64_t *i64 = (int64_t *)malloc(sizeof(int64_t) * (n ? n : 1));
    int rc = rp_sim_view((rp_sim *)h->p, v, (uint8_t *)sd, i64);
    for (uint32_t i = 0; rc == 0 && i < n; i++) ((double *)id)[i] = (double)i64[i];
    free(i64);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "status", st);
    napi_set_named_property(env, out, "inc", inc);
    return out;
}

/* simCensus(handle, n, observe: Uint8Array(n) | null) -> {observers, status: Uint32Array(4n),
 * inRing, atMax: Uint32Array(n), maxInc: Float64Array(n) (as simView's inc), behind: Uint32Array(n)} */
static napi_value js_sim_census(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t n = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &n));
    size_t no = 0;
    const uint8_t *observe = (const uint8_t *)typed_data(env, argv[2], napi_uint8_array, &no);
    napi_valuetype vt = napi_undefined;
    napi_typeof(env, argv[2], &vt);
    if ((vt != napi_null && vt != napi_undefined && !observe && n) || (observe && no != n)) {
        napi_throw_type_error(env, NULL, "observe: a Uint8Array with one entry per node, or null");
        return NULL;
    }
    void *sd = NULL, *rd = NULL, *ad = NULL, *bd = NULL, *md = NULL;
    napi_value st = new_typed(env, napi_uint32_array, 4 * (size_t)n, 4, &sd);
    napi_value ring = new_typed(env, napi_uint32_array, n, 4, &rd);
    napi_value at = new_typed(env, napi_uint32_array, n, 4, &ad);
    napi_value behind = new_typed(env, napi_uint32_array, n, 4, &bd);
    napi_value mx = new_typed(env, napi_float64_array, n, 8, &md);
    int64_t *i64 = (int64_t *)malloc(sizeof(int64_t) * (n ? n : 1));
    uint32_t n_obs = 0;
    int rc = rp_sim_census((rp_sim *)h->p, observe, NULL, &n_obs, (uint32_t *)sd, (uint32_t *)rd, i64, (uint32_t *)ad,
                           (uint32_t *)bd);
    for (uint32_t i = 0; rc == 0 && i < n; i++) ((double *)md)[i] = (double)i64[i];
    free(i64);
    RP_OK(rc);
    napi_value out, nv;
    napi_create_object(env, &out);
    napi_create_uint32(env, n_obs, &nv);
    napi_set_named_property(env, out, "observers", nv);
    napi_set_named_property(env, out, "status", st);
    napi_set_named_property(env, out, "inRing", ring);
    napi_set_named_property(env, out, "maxInc", mx);
    napi_set_named_property(env, out, "atMax", at);
    napi_set_named_property(env, out, "behind", behind);
    return out;
}

static napi_value js_sim_sides(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t n = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &n));
    void *d = NULL;
    napi_value out = new_typed(env, napi_uint8_array, n, 1, &d);
    RP_OK(rp_sim_sides((rp_sim *)h->p, (uint8_t *)d));
    return out;
}

/* rp_sim_side_summary: {nodes, ckMin, ckMax: Uint32Array(256), crossPingable: Float64Array(256)} */
static napi_value js_sim_side_summary(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    void *nd = NULL, *lo = NULL, *hi = NULL, *cd = NULL;
    napi_value nodes = new_typed(env, napi_uint32_array, 256, 4, &nd);
    napi_value ck_min = new_typed(env, napi_uint32_array, 256, 4, &lo);
    napi_value ck_max = new_typed(env, napi_uint32_array, 256, 4, &hi);
    napi_value cross = new_typed(env, napi_float64_array, 256, 8, &cd);
    uint64_t c64[256];
    RP_OK(rp_sim_side_summary((rp_sim *)h->p, (uint32_t *)nd, (uint32_t *)lo, (uint32_t *)hi, c64));
    for (int i = 0; i < 256; i++) ((double *)cd)[i] = (double)c64[i];
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "nodes", nodes);
    napi_set_named_property(env, out, "ckMin", ck_min);
    napi_set_named_property(env, out, "ckMax", ck_max);
    napi_set_named_property(env, out, "crossPingable", cross);
    return out;
}

static napi_value js_sim_timeline_enable(napi_env env, napi_callback_info info) {
    ARGS(2);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t cap = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &cap));
    RP_OK(rp_sim_timeline_enable((rp_sim *)h->p, cap));
    return NULL;
}

/* simTimelineRead(handle, n, cap) -> {count, firstRound, recs: Float64Array(15 * count), per record
 * {round, observers, ckMin, ckMax, pairs[4], inRing, unmet, falseFaulty, stats[4]} (every field is at
 * most n^2 or a traffic count: exact in a double), firstSeen: Uint32Array(3n)} */
static napi_value js_sim_timeline_read(napi_env env, napi_callback_info info) {
    ARGS(3);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint32_t n = 0, cap = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &n));
    NAPI_OK(napi_get_value_uint32(env, argv[2], &cap));
    rp_sim_round_rec *recs = (rp_sim_round_rec *)malloc(sizeof(rp_sim_round_rec) * (cap ? cap : 1));
    void *fd = NULL;
    napi_value fs = new_typed(env, napi_uint32_array, 3 * (size_t)n, 4, &fd);
    memset(fd, 0xFF, 12 * (size_t)n);
    uint32_t cnt = 0;
    uint64_t first = 0;
    int rc = rp_sim_timeline_read((rp_sim *)h->p, recs, cap, &cnt, &first, (uint32_t *)fd);
    if (rc) {
        free(recs);
        RP_OK(rc);
    }
    void *rd = NULL;
    napi_value arr = new_typed(env, napi_float64_array, 15 * (size_t)cnt, 8, &rd);
    for (uint32_t i = 0; i < cnt; i++) {
        double *o = (double *)rd + 15 * (size_t)i;
        const rp_sim_round_rec *r = recs + i;
        o[0] = (double)r->round;
        o[1] = (double)r->observers;
        o[2] = (double)r->ck_min;
        o[3] = (double)r->ck_max;
        for (int k = 0; k < 4; k++) o[4 + k] = (double)r->pairs[k];
        o[8] = (double)r->in_ring;
        o[9] = (double)r->unmet;
        o[10] = (double)r->false_faulty;
        for (int k = 0; k < 4; k++) o[11 + k] = (double)r->stats[k];
    }
    free(recs);
    napi_value out, v;
    napi_create_object(env, &out);
    napi_create_uint32(env, cnt, &v);
    napi_set_named_property(env, out, "count", v);
    napi_create_double(env, (double)first, &v);
    napi_set_named_property(env, out, "firstRound", v);
    napi_set_named_property(env, out, "recs", arr);
    napi_set_named_property(env, out, "firstSeen", fs);
    return out;
}

static napi_value js_sim_converged(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    int c = 0;
    RP_OK(rp_sim_converged((rp_sim *)h->p, &c));
    return make_bool(env, c);
}

static napi_value js_sim_stats(napi_env env, napi_callback_info info) {
    ARGS(1);
    handle_t *h = get_handle(env, argv[0], 3);
    if (!h) return NULL;
    uint64_t s[4] = {0, 0, 0, 0};
    RP_OK(rp_sim_stats((rp_sim *)h->p, s));
    static const char *names[4] = {"pings", "pingReqs", "fullSyncs", "applied"};
    napi_value out;
    napi_create_object(env, &out);
    for (int i = 0; i < 4; i++) {
        napi_value v;
        napi_create_double(env, (double)s[i], &v);
        napi_set_named_property(env, out, names[i], v);
    }
    return out;
}

/* ------------------------------------------------------------------ module */
/* ------------------------------------------------------------------ wire bodies */
/* the typed array at obj[key] (NULL when absent / null); *n its length */
static void *prop_typed(napi_env env, napi_value obj, const char *key, napi_typedarray_type t, size_t *n) {
    *n = 0;
    if (is_nullish(env, obj)) return NULL;
    napi_value v;
    if (napi_get_named_property(env, obj, key, &v) != napi_ok || is_nullish(env, v)) return NULL;
    return typed_data(env, v, t, n);
}

/* Incarnation numbers arrive as doubles (JS Numbers). Converting NaN, +-Inf or a value outside
 * int64 to int64_t is undefined behaviour in C, so those are rejected with a TypeError (NaN only
 * where it stands for "absent": nan_is_min). Returns NULL with the exception pending. */
static int64_t *f64_to_i64(napi_env env, const double *d, size_t n, int nan_is_min, const char *what) {
    int64_t *o = (int64_t *)malloc(sizeof(int64_t) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        const double x = d[i];
        if (nan_is_min && x != x) {
            o[i] = INT64_MIN;
        } else if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) { /* NaN, Inf, range */
            char msg[160];
            snprintf(msg, sizeof msg, "%s[%zu] is not a finite number within int64 range", what, i);
            free(o);
            napi_throw_type_error(env, NULL, msg);
            return NULL;
        } else {
            o[i] = (int64_t)x;
        }
    }
    return o;
}

/* wireEncode(h, msgRecOff Uint32Array, recs {addr, src, status, inc, srcInc?, ids?}, form, body,
 * hdr {checksum?, source?, sourceInc?, target?, pingStatus?, app?}) -> {bytes: Uint8Array,
 * off: Float64Array}: JSON.stringify of the gossip bodies (dissemination.js:163-170, ping /
 * ping-req / join bodies) on the device (rp_wire_encode). inc / srcInc are Float64Array (srcInc
 * NaN = absent); src RP_NULL_ID = absent; an ids row starting with 0 = absent. */
static napi_value js_wire_encode(napi_env env, napi_callback_info info) {
    ARGS(6);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    size_t nro = 0, na = 0, ns = 0, nst = 0, ni = 0, nsi = 0, nid = 0;
    const uint32_t *ro = (const uint32_t *)typed_data(env, argv[1], napi_uint32_array, &nro);
    if (!ro || nro < 1) {
        napi_throw_type_error(env, NULL, "wireEncode expects msgRecOff Uint32Array(n_msgs + 1)");
        return NULL;
    }
    const uint32_t n_msgs = (uint32_t)(nro - 1), n_rec = ro[n_msgs];
    const uint32_t *addr = (const uint32_t *)prop_typed(env, argv[2], "addr", napi_uint32_array, &na);
    const uint32_t *src = (const uint32_t *)prop_typed(env, argv[2], "src", napi_uint32_array, &ns);
    const uint8_t *st = (const uint8_t *)prop_typed(env, argv[2], "status", napi_uint8_array, &nst);
    const double *incd = (const double *)prop_typed(env, argv[2], "inc", napi_float64_array, &ni);
    const double *sincd = (const double *)prop_typed(env, argv[2], "srcInc", napi_float64_array, &nsi);
    const uint8_t *ids = (const uint8_t *)prop_typed(env, argv[2], "ids", napi_uint8_array, &nid);
    if (na < n_rec || ns < n_rec || nst < n_rec || ni < n_rec || (sincd && nsi < n_rec) || (ids && nid < 36ull * n_rec)) {
        napi_throw_type_error(env, NULL, "wireEncode: record columns shorter than msgRecOff says");
        return NULL;
    }
    int32_t form = 0, body = 0;
    NAPI_OK(napi_get_value_int32(env, argv[3], &form));
    NAPI_OK(napi_get_value_int32(env, argv[4], &body));
    size_t hck = 0, hs = 0, hsi = 0, ht = 0, hp = 0;
    const uint32_t *ck = (const uint32_t *)prop_typed(env, argv[5], "checksum", napi_uint32_array, &hck);
    const uint32_t *ms = (const uint32_t *)prop_typed(env, argv[5], "source", napi_uint32_array, &hs);
    const double *msid = (const double *)prop_typed(env, argv[5], "sourceInc", napi_float64_array, &hsi);
    const uint32_t *tg = (const uint32_t *)prop_typed(env, argv[5], "target", napi_uint32_array, &ht);
    const uint8_t *ps = (const uint8_t *)prop_typed(env, argv[5], "pingStatus", napi_uint8_array, &hp);
    if ((ck && hck < n_msgs) || (ms && hs < n_msgs) || (msid && hsi < n_msgs) || (tg && ht < n_msgs) ||
        (ps && hp < n_msgs)) {
        napi_throw_type_error(env, NULL, "wireEncode: header columns shorter than the message count");
        return NULL;
    }
    /* the join response's app name, any length (its byte length first, then the bytes) */
    char *app = NULL;
    size_t app_len = 0;
    if (!is_nullish(env, argv[5])) {
        napi_value av;
        if (napi_get_named_property(env, argv[5], "app", &av) == napi_ok && !is_nullish(env, av)) {
            NAPI_OK(napi_get_value_string_utf8(env, av, NULL, 0, &app_len));
            app = (char *)malloc(app_len + 1);
            size_t got = 0;
            NAPI_OK(napi_get_value_string_utf8(env, av, app, app_len + 1, &got));
            app_len = got;
        }
    }
    int64_t *inc = f64_to_i64(env, incd, n_rec, 0, "wireEncode: inc");
    int64_t *sinc = (inc && sincd) ? f64_to_i64(env, sincd, n_rec, 1, "wireEncode: srcInc") : NULL;
    int64_t *msi = (inc && (!sincd || sinc) && msid) ? f64_to_i64(env, msid, n_msgs, 0, "wireEncode: sourceInc") : NULL;
    if (!inc || (sincd && !sinc) || (msid && !msi)) {
        free(inc);
        free(sinc);
        free(msi);
        free(app);
        return NULL;
    }
    rp_wire_records R = {addr, src, st, inc, sinc, ids};
    rp_wire_headers H = {ck, ms, msi, tg, ps, app_len ? app : NULL, (uint32_t)app_len};
    void *od = NULL, *bd = NULL;
    napi_value off = new_typed(env, napi_float64_array, n_msgs + 1, 8, &od);
    uint64_t *o64 = (uint64_t *)malloc(sizeof(uint64_t) * (n_msgs + 1));
    int rc = rp_wire_encode((rp_members *)h->p, n_msgs, ro, &R, form, body, &H, NULL, 0, o64);
    napi_value bytes = NULL;
    if (rc == 0) {
        bytes = new_typed(env, napi_uint8_array, o64[n_msgs] ? o64[n_msgs] : 1, 1, &bd);
        rc = rp_wire_encode((rp_members *)h->p, n_msgs, ro, &R, form, body, &H, (uint8_t *)bd, o64[n_msgs], o64);
    }
    for (uint32_t j = 0; rc == 0 && j <= n_msgs; j++) ((double *)od)[j] = (double)o64[j];
    free(inc);
    free(sinc);
    free(msi);
    free(o64);
    free(app);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "bytes", bytes);
    napi_set_named_property(env, out, "off", off);
    return out;
}

/* wireDecode(h, bytes Uint8Array, msgOff Float64Array(n + 1), recCap) -> {recOff, addr, src, status,
 * inc, srcInc (NaN absent), idOff, addrOff, addrLen, err, checksum, source, sourceInc (NaN absent),
 * target, pingStatus}: safeParse + the bodies' members on the device (rp_wire_decode). */
static napi_value js_wire_decode(napi_env env, napi_callback_info info) {
    ARGS(4);
    handle_t *h = get_handle(env, argv[0], 2);
    if (!h) return NULL;
    size_t nb = 0, no = 0;
    const char *buf = (const char *)typed_data(env, argv[1], napi_uint8_array, &nb);
    const double *offd = (const double *)typed_data(env, argv[2], napi_float64_array, &no);
    uint32_t cap = 0;
    NAPI_OK(napi_get_value_uint32(env, argv[3], &cap));
    if (!offd || no < 1) {
        napi_throw_type_error(env, NULL, "wireDecode expects msgOff Float64Array(n_msgs + 1)");
        return NULL;
    }
    const uint32_t n = (uint32_t)(no - 1);
    uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (n + 1));
    for (uint32_t j = 0; j <= n; j++) off[j] = (uint64_t)offd[j];
    if (off[n] > nb) {
        free(off);
        napi_throw_range_error(env, NULL, "wireDecode: msgOff past the buffer");
        return NULL;
    }
    const size_t c = cap ? cap : 1, m1 = n ? n : 1;
    void *p_ro, *p_a, *p_s, *p_st, *p_i, *p_si, *p_id, *p_ao, *p_al, *p_err, *p_ck, *p_ms, *p_msi, *p_tg, *p_ps;
    napi_value ro = new_typed(env, napi_uint32_array, n + 1, 4, &p_ro);
    napi_value a = new_typed(env, napi_uint32_array, c, 4, &p_a);
    napi_value s2 = new_typed(env, napi_uint32_array, c, 4, &p_s);
    napi_value st = new_typed(env, napi_uint8_array, c, 1, &p_st);
    napi_value inc = new_typed(env, napi_float64_array, c, 8, &p_i);
    napi_value sinc = new_typed(env, napi_float64_array, c, 8, &p_si);
    napi_value idoff = new_typed(env, napi_float64_array, c, 8, &p_id);
    napi_value aoff = new_typed(env, napi_float64_array, c, 8, &p_ao);
    napi_value alen = new_typed(env, napi_uint32_array, c, 4, &p_al);
    napi_value err = new_typed(env, napi_float64_array, m1, 8, &p_err);
    napi_value ck = new_typed(env, napi_uint32_array, m1, 4, &p_ck);
    napi_value ms = new_typed(env, napi_uint32_array, m1, 4, &p_ms);
    napi_value msi = new_typed(env, napi_float64_array, m1, 8, &p_msi);
    napi_value tg = new_typed(env, napi_uint32_array, m1, 4, &p_tg);
    napi_value ps = new_typed(env, napi_uint8_array, m1, 1, &p_ps);
    int64_t *i64 = (int64_t *)malloc(8 * c), *si64 = (int64_t *)malloc(8 * c), *msi64 = (int64_t *)malloc(8 * m1);
    uint64_t *id64 = (uint64_t *)malloc(8 * c), *ao64 = (uint64_t *)malloc(8 * c), *e64 = (uint64_t *)malloc(8 * m1);
    rp_wire_records_out R = {(uint32_t *)p_a, (uint32_t *)p_s, (uint8_t *)p_st, i64, si64, id64, ao64, (uint32_t *)p_al};
    rp_wire_headers_out H = {(uint32_t *)p_ck, (uint32_t *)p_ms, msi64, (uint32_t *)p_tg, (uint8_t *)p_ps};
    const int rc = rp_wire_decode((rp_members *)h->p, buf, off, n, (uint32_t *)p_ro, cap, &R, &H, e64);
    if (rc == 0) {
        const uint32_t k = ((uint32_t *)p_ro)[n] < cap ? ((uint32_t *)p_ro)[n] : cap;
        for (uint32_t r = 0; r < k; r++) {
            ((double *)p_i)[r] = (double)i64[r];
            ((double *)p_si)[r] = si64[r] == INT64_MIN ? NAN : (double)si64[r];
            ((double *)p_id)[r] = id64[r] == UINT64_MAX ? -1 : (double)id64[r];
            ((double *)p_ao)[r] = (double)ao64[r];
        }
        for (uint32_t j = 0; j < n; j++) {
            ((double *)p_err)[j] = (double)e64[j];
            ((double *)p_msi)[j] = msi64[j] == INT64_MIN ? NAN : (double)msi64[j];
        }
    }
    free(off); free(i64); free(si64); free(msi64); free(id64); free(ao64); free(e64);
    RP_OK(rc);
    napi_value out;
    napi_create_object(env, &out);
    const char *names[] = {"recOff", "addr", "src", "status", "inc", "srcInc", "idOff", "addrOff", "addrLen", "err",
                           "checksum", "source", "sourceInc", "target", "pingStatus"};
    napi_value vals[] = {ro, a, s2, st, inc, sinc, idoff, aoff, alen, err, ck, ms, msi, tg, ps};
    for (size_t i = 0; i < sizeof(vals) / sizeof(vals[0]); i++) napi_set_named_property(env, out, names[i], vals[i]);
    return out;
}

static napi_value init(napi_env env, napi_value exports) {
    static const struct {
        const char *name;
        napi_callback fn;
    } fns[] = {
        {"version", js_version},
        {"deviceCount", js_device_count},
        {"hash32", js_hash32},
        {"destroy", js_destroy},
        {"ringCreate", js_ring_create},
        {"ringAddRemove", js_ring_add_remove},
        {"ringChecksum", js_ring_checksum},
        {"ringChecksumString", js_ring_checksum_string},
        {"ringServerCount", js_ring_server_count},
        {"ringService", js_ring_service},
        {"ringLookup1", js_ring_lookup1},
        {"ringLookupN1", js_ring_lookupn1},
        {"ringTokenCount", js_ring_token_count},
        {"ringHasServer", js_ring_has_server},
        {"ringServers", js_ring_servers},
        {"ringOwnerName", js_ring_owner_name},
        {"ringLookup", js_ring_lookup},
        {"ringLookupN", js_ring_lookupn},
        {"ringLookupNHashes", js_ring_lookupn_hashes},
        {"ringGroupKeys", js_ring_group_keys},
        {"membersCreate", js_members_create},
        {"membersIntern", js_members_intern},
        {"membersSetLocal", js_members_set_local},
        {"membersUpdate", js_members_update},
        {"membersSet", js_members_set},
        {"membersChecksum", js_members_checksum},
        {"membersComputeChecksum", js_members_compute_checksum},
        {"membersChecksumString", js_members_checksum_string},
        {"membersDump", js_members_dump},
        {"membersDampConfigure", js_members_damp_configure},
        {"membersDampLast", js_members_damp_last},
        {"membersDampDecay", js_members_damp_decay},
        {"membersDampDump", js_members_damp_dump},
        {"simCreate", js_sim_create},
        {"simStep", js_sim_step},
        {"simRound", js_sim_round},
        {"simChecksums", js_sim_checksums},
        {"simView", js_sim_view},
        {"simConverged", js_sim_converged},
        {"simStats", js_sim_stats},
        {"wireEncode", js_wire_encode},
        {"wireDecode", js_wire_decode},
    };
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); i++) {
        napi_value f;
        napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f);
        napi_set_named_property(env, exports, fns[i].name, f);
    }
    /* Entry points added after the enumerable list above was pinned (tests/test_js.py compares
     * Object.keys of the addon with it): defined as non-enumerable properties, called the same
     * way (native.ringSnapshot(...)). */
    const napi_property_descriptor later[] = {
        {"ringSnapshot", NULL, js_ring_snapshot, NULL, NULL, NULL, napi_default, NULL},
        {"ringSnapInfo", NULL, js_ring_snap_info, NULL, NULL, NULL, napi_default, NULL},
        {"ringMovedKeys", NULL, js_ring_moved_keys, NULL, NULL, NULL, napi_default, NULL},
        {"ringHandoff", NULL, js_ring_handoff, NULL, NULL, NULL, napi_default, NULL},
        {"ringRouteViews", NULL, js_ring_route_views, NULL, NULL, NULL, napi_default, NULL},
        {"ringRouteShare", NULL, js_ring_route_share, NULL, NULL, NULL, napi_default, NULL},
        {"ringOwnerLoad", NULL, js_ring_owner_load, NULL, NULL, NULL, napi_default, NULL},
        {"ringOwnerShare", NULL, js_ring_owner_share, NULL, NULL, NULL, napi_default, NULL},
        {"ringMovedRanges", NULL, js_ring_moved_ranges, NULL, NULL, NULL, napi_default, NULL},
        {"ringSnapDump", NULL, js_ring_snap_dump, NULL, NULL, NULL, napi_default, NULL},
        {"simCensus", NULL, js_sim_census, NULL, NULL, NULL, napi_default, NULL},
        {"simSides", NULL, js_sim_sides, NULL, NULL, NULL, napi_default, NULL},
        {"simSideSummary", NULL, js_sim_side_summary, NULL, NULL, NULL, napi_default, NULL},
        {"simTimelineEnable", NULL, js_sim_timeline_enable, NULL, NULL, NULL, napi_default, NULL},
        {"simTimelineRead", NULL, js_sim_timeline_read, NULL, NULL, NULL, napi_default, NULL},
    };
    napi_define_properties(env, exports, sizeof(later) / sizeof(later[0]), later);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
