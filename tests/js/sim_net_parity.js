// sim_net_parity.js — replays partition cases of tests/golden/sim_net_golden.json (the reference
// modules under tests/golden/ref_sim_net.js) through the N-API GossipSim of ringpop-node_amd/js:
// every live node's checksum and every node's side after every round, and sideSummary() against
// the checksums and sides of the same round. in.json (from tests/test_js_sim_net_gpu.py) adds each
// case's names, inc0 and the nodes that are up and have not left after each round (observers).
// Prints one JSON line.
'use strict';
var fs = require('fs');
var path = require('path');
var amd = require(path.join(__dirname, '..', '..', 'ringpop-node_amd', 'js'));

var input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var fails = [], checks = 0;
function same(a, b) { return JSON.stringify(Array.from(a)) === JSON.stringify(b); }
input.cases.forEach(function (c) {
    var sim = new amd.GossipSim(c.names, {inc0: c.inc0, dead: c.dead, seed: c.seed,
        suspicionRounds: c.suspRounds, now0: c.now0, events: c.events});
    c.checksums.forEach(function (want, r) {
        sim.step(1);
        checks += 3;
        if (!same(sim.checksums(), want)) { fails.push(c.name + ' checksums, round ' + r); }
        if (!same(sim.sides(), c.sides[r])) { fails.push(c.name + ' sides, round ' + r); }
        var s = sim.sideSummary();
        var nodes = new Array(256).fill(0), lo = new Array(256).fill(0xFFFFFFFF), hi = new Array(256).fill(0);
        c.observers[r].forEach(function (v) {
            var k = c.sides[r][v];
            nodes[k]++;
            lo[k] = Math.min(lo[k], want[v]);
            hi[k] = Math.max(hi[k], want[v]);
        });
        var ok = same(s.nodes, nodes) && same(s.ckMin, lo) && same(s.ckMax, hi) && s.settled.length === 256 &&
            s.settled.every(function (x, k) { return x === (lo[k] === hi[k] && s.crossPingable[k] === 0); });
        // before the first cut nothing is across
        if (c.sides.slice(0, r + 1).every(function (row) { return row.every(function (x) { return x === 0; }); }) &&
            c.dead.every(function (d) { return !d; }) && r < c.firstEvent) {
            ok = ok && s.crossPingable.every(function (x) { return x === 0; });
        }
        if (!ok) { fails.push(c.name + ' sideSummary, round ' + r); }
    });
    var last = sim.sideSummary();
    checks++;
    if (c.crossFinal !== null && !same(last.crossPingable, c.crossFinal)) { fails.push(c.name + ' crossPingable at the end'); }
    sim.destroy();
});
['side', 'kind'].forEach(function (what) {
    checks++;
    try {
        var bad = new amd.GossipSim(input.cases[0].names, {inc0: input.cases[0].inc0, seed: 1,
            events: [what === 'side' ? [0, 'side', 0, 256] : [0, 6, 0]]});
        bad.destroy();
        fails.push('a bad ' + what + ' was accepted');
    } catch (e) {
        if (!/bad event/.test(e.message)) { fails.push('a bad ' + what + ': ' + e.message); }
    }
});
process.stdout.write(JSON.stringify({checks: checks, fails: fails.slice(0, 20), nfail: fails.length}) + '\n');
