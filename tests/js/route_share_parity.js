// route_share_parity.js — routeShare through the N-API HashRing of ringpop-node_amd/js against the
// Python binding's result for the same ring, views and truth (tests/test_js_route_share_gpu.py
// computes it; the Python result is itself pinned against the numpy model in
// tests/test_ring_route_share_gpu.py). Prints one JSON line.
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
    ring.addRemoveServers(c.servers, []);
    var r = c.truth === null ? ring.routeShare(c.views) : ring.routeShare(c.views, c.truth);
    eq(c.name + ' wrong', r.wrong, c.want.wrong);
    eq(c.name + ' lost', r.lost, c.want.lost);
    eq(c.name + ' disputed', r.disputed, c.want.disputed);
    var raw = amd.native.ringRouteShare(ring._h, c.views, c.truth);
    eq(c.name + ' typed', [raw.wrong instanceof Float64Array, raw.lost instanceof Float64Array,
        raw.posWrong instanceof Uint32Array, raw.wrong.length, raw.posWrong.length],
    [true, true, true, c.views.length, c.want.posWrong.length]);
    eq(c.name + ' posWrong', Array.from(raw.posWrong), c.want.posWrong);
    var z = ring.routeShare([]);
    eq(c.name + ' no views', z, {wrong: [], lost: [], disputed: 0});
    ring.destroy();
});

var empty = new amd.HashRing({});
eq('empty ring', empty.routeShare([['10.0.0.1:1'], []]), {wrong: [0, 0], lost: [0, 0], disputed: 0});
empty.destroy();

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
