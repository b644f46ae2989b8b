// load_parity.js — ownerLoad / ownerShare through the N-API HashRing of ringpop-node_amd/js
// against values tests/test_js_load_gpu.py computes from the CPU oracle for the same ring and
// keys. Prints one JSON line.
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
    eq(c.name + ' empty load', ring.ownerLoad(c.keys, c.n), {});
    eq(c.name + ' empty share', ring.ownerShare(), {});
    ring.addRemoveServers(c.initial, []);
    ring.addRemoveServers(c.add, c.remove);
    var load = ring.ownerLoad(c.keys, c.n);
    eq(c.name + ' load servers', Object.keys(load), c.want.servers);
    eq(c.name + ' load', load, c.want.load);
    eq(c.name + ' load is plain arrays of numbers', Object.keys(load).every(function (s) {
        return Array.isArray(load[s]) && load[s].length === Math.max(c.n, 1) &&
            load[s].every(function (x) { return typeof x === 'number'; });
    }), true);
    var share = ring.ownerShare();
    eq(c.name + ' share servers', Object.keys(share), c.want.servers);
    eq(c.name + ' share', share, c.want.share);
    eq(c.name + ' share sums to 2^32', Object.keys(share).reduce(function (a, s) { return a + share[s]; }, 0), 4294967296);
    eq(c.name + ' no keys', ring.ownerLoad([], c.n)[c.want.servers[0]], c.want.load[c.want.servers[0]].map(function () { return 0; }));
    ring.destroy();
});

console.log(JSON.stringify({nfail: fails.length, fails: fails.slice(0, 10), checks: checks}));
