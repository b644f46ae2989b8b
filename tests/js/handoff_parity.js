// handoff_parity.js — the hand-off plan through the N-API HashRing of ringpop-node_amd/js against
// the Python binding's result for the same ring change and keys (tests/test_js_handoff_gpu.py
// computes it; the Python result is itself pinned against the CPU oracle and the numpy model in
// tests/test_ring_handoff_gpu.py). Prints one JSON line.
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
    var snap = ring.snapshot();
    var none = ring.handoffPlan(c.keys, snap, c.n);
    eq(c.name + ' no change', [none.count, none.dests.length, Array.from(none.groupOff)], [0, 0, [0]]);
    ring.addRemoveServers(c.add, c.remove);
    var p = ring.handoffPlan(c.keys, snap, c.n);
    eq(c.name + ' count', p.count, c.want.keyIdx.length);
    eq(c.name + ' typed', [p.dests instanceof Uint32Array, p.groupOff instanceof Uint32Array, p.keyIdx instanceof Uint32Array,
        p.src instanceof Uint32Array, p.slot instanceof Uint8Array, p.groupOff.length, p.src.length, p.slot.length],
        [true, true, true, true, true, p.dests.length + 1, p.count, p.count]);
    eq(c.name + ' groupOff', Array.from(p.groupOff), c.want.groupOff);
    eq(c.name + ' keyIdx', Array.from(p.keyIdx), c.want.keyIdx);
    eq(c.name + ' slot', Array.from(p.slot), c.want.slot);
    var names = ring.handoffNames(c.keys, p);
    eq(c.name + ' dests', names.map(function (x) { return x.dest; }), c.want.dests);
    eq(c.name + ' transfers', names.map(function (x) {
        return x.transfers.map(function (t) { return [t.key, t.src]; });
    }), c.want.transfers);
    var mine = ring.handoffPlan(c.keys, snap, c.n, c.whoami);
    eq(c.name + ' whoami', [mine.count, Array.from(mine.keyIdx), Array.from(mine.groupOff)],
        [c.want.mine.keyIdx.length, c.want.mine.keyIdx, c.want.mine.groupOff]);
    eq(c.name + ' whoami src', ring.handoffNames(c.keys, mine).every(function (x) {
        return x.transfers.every(function (t) { return t.src === c.whoami; });
    }), true);
    eq(c.name + ' unknown whoami', ring.handoffPlan(c.keys, snap, c.n, 'nobody:1').count, 0);
    snap.destroy();
    ring.destroy();
});

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
