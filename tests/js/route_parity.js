// route_parity.js — routeViews through the N-API HashRing of ringpop-node_amd/js against the
// Python binding's result for the same ring, keys, views and truth (tests/test_js_route_gpu.py
// computes it; the Python result is itself pinned against the numpy model in
// tests/test_ring_route_gpu.py). Prints one JSON line.
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
    ring.addRemoveServers(c.servers, []);
    var r = c.truth === null ? ring.routeViews(c.keys, c.views) : ring.routeViews(c.keys, c.views, c.truth);
    eq(c.name + ' owners', r.owners, c.want.owners);
    eq(c.name + ' truth', r.truth, c.want.truth);
    eq(c.name + ' wrong', r.wrong, c.want.wrong);
    eq(c.name + ' lost', r.lost, c.want.lost);
    var raw = amd.native.ringRouteViews(ring._h, ring._customHash ? ring._hashes(c.keys) : c.keys, c.views, c.truth);
    eq(c.name + ' typed', [raw.wrong instanceof Float64Array, raw.lost instanceof Float64Array,
        raw.keyWrong instanceof Uint32Array, raw.truthOwner instanceof Uint32Array, raw.owners instanceof Uint32Array,
        raw.views, raw.owners.length, raw.keyWrong.length],
    [true, true, true, true, true, c.views.length, c.keys.length * c.views.length, c.keys.length]);
    eq(c.name + ' keyWrong', Array.from(raw.keyWrong), c.want.keyWrong);
    var e = ring.routeViews([], c.views, c.truth === null ? undefined : c.truth);
    eq(c.name + ' no keys', [e.owners.length, e.wrong], [0, c.views.map(function () { return 0; })]);
    var z = ring.routeViews(c.keys.slice(0, 3), []);
    eq(c.name + ' no views', [z.owners, z.wrong, z.truth.length], [[[], [], []], [], 3]);
    ring.destroy();
});

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
