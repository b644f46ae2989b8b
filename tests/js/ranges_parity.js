// ranges_parity.js — movedRanges / movedRangeNames / snap.dump() through the N-API HashRing of
// ringpop-node_amd/js against the Python binding's result for the same ring change
// (tests/test_js_ranges_gpu.py computes it; the Python result is itself pinned against the CPU
// oracle in tests/test_ring_ranges_gpu.py). Prints one JSON line.
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
    var ring = new amd.HashRing({});
    ring.addRemoveServers(c.initial, []);
    var snap = ring.snapshot();
    var same = ring.movedRanges(snap, c.n);
    eq(c.name + ' no change', [same.count, same.movedHashes, same.lo.length], [0, 0, 0]);
    ring.addRemoveServers(c.add, c.remove);
    var m = ring.movedRanges(snap, c.n);
    var w = Math.max(c.n, 1);
    eq(c.name + ' count', m.count, c.want.lo.length);
    eq(c.name + ' movedHashes', m.movedHashes, c.want.movedHashes);
    eq(c.name + ' typed', [m.lo instanceof Uint32Array, m.hi instanceof Uint32Array, m.before instanceof Uint32Array,
        m.after instanceof Uint32Array, m.hi.length, m.before.length, m.after.length],
        [true, true, true, true, m.count, m.count * w, m.count * w]);
    eq(c.name + ' lo', Array.from(m.lo), c.want.lo);
    eq(c.name + ' hi', Array.from(m.hi), c.want.hi);
    var names = ring.movedRangeNames(m, c.n);
    eq(c.name + ' names lo hi', names.map(function (x) { return [x.lo, x.hi]; }),
        c.want.lo.map(function (l, j) { return [l, c.want.hi[j]]; }));
    eq(c.name + ' before', names.map(function (x) { return x.before; }), c.want.before);
    eq(c.name + ' after', names.map(function (x) { return x.after; }), c.want.after);
    var d = snap.dump();
    eq(c.name + ' dump typed', [d.tokens instanceof Uint32Array, d.owners instanceof Uint32Array], [true, true]);
    eq(c.name + ' dump tokens', Array.from(d.tokens), c.want.tokens);
    eq(c.name + ' dump owners', Array.from(d.owners).map(function (id) { return ring.ownerName(id); }), c.want.owners);
    eq(c.name + ' not enumerable', [Object.keys(amd.native).indexOf('ringMovedRanges'),
        Object.keys(amd.native).indexOf('ringSnapDump'), typeof amd.native.ringMovedRanges], [-1, -1, 'function']);
    ring.destroy();
    eq(c.name + ' dump after ring.destroy', snap.dump().tokens.length, c.want.tokens.length);
    snap.destroy();
});

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
