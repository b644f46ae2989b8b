// moved_parity.js — ring snapshots and movedKeys through the N-API HashRing of
// ringpop-node_amd/js against the Python binding's result for the same ring change and keys
// (tests/test_js_moved_gpu.py computes it; the Python result is itself pinned against the CPU
// oracle in tests/test_ring_moved_gpu.py). Prints one JSON line.
'use strict';
var fs = require('fs');
var path = require('path');
var amd = require(path.join(__dirname, '..', '..', 'ringpop-node_amd', 'js'));

var input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var fails = [];
var checks = 0;

function eq(what, got, want) {
    checks++;
    if (JSON.stringify(got) !== JSON.stringify(want)) {
        fails.push({what: what, got: String(JSON.stringify(got)).slice(0, 200), want: String(JSON.stringify(want)).slice(0, 200)});
    }
}

input.cases.forEach(function (c) {
    var opts = c.reverseHash ? {hashFunc: function (s) { return amd.hash32(String(s).split('').reverse().join('')); }} : {};
    var ring = new amd.HashRing(opts);
    ring.addRemoveServers(c.initial, []);
    // (the snapshot keeps the device checksum: farmhash32 of the checksum string)
    var before = {checksum: amd.hash32(amd.native.ringChecksumString(ring._h))};
    var snap = ring.snapshot();
    eq(c.name + ' no change', ring.movedKeys(c.keys, snap, c.n).count, 0);
    ring.addRemoveServers(c.add, c.remove);
    var m = ring.movedKeys(c.keys, snap, c.n);
    eq(c.name + ' count', m.count, c.want.idx.length);
    eq(c.name + ' idx', Array.from(m.idx), c.want.idx);
    eq(c.name + ' typed', [m.idx instanceof Uint32Array, m.before instanceof Uint32Array, m.after instanceof Uint32Array,
        m.before.length, m.after.length], [true, true, true, m.count * Math.max(c.n, 1), m.count * Math.max(c.n, 1)]);
    var names = ring.movedNames(c.keys, m, c.n);
    eq(c.name + ' keys', names.map(function (x) { return x.key; }), c.want.idx.map(function (i) { return c.keys[i]; }));
    eq(c.name + ' before', names.map(function (x) { return x.before; }), c.want.before);
    eq(c.name + ' after', names.map(function (x) { return x.after; }), c.want.after);
    var info = snap.info();
    eq(c.name + ' info', [info.servers, info.checksum], [c.initial.length, before.checksum]);
    eq(c.name + ' info tokens', info.tokens, c.want.tokens);
    // the snapshot outlives the ring; destroying it twice is harmless
    ring.destroy();
    eq(c.name + ' info after ring.destroy', snap.info().servers, c.initial.length);
    snap.destroy();
    snap.destroy();
    var threw = false;
    try { snap.info(); } catch (e) { threw = true; }
    eq(c.name + ' destroyed snapshot is refused', threw, true);
});

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
