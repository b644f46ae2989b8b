// timeline_parity.js — GossipSim.timelineEnable / timeline of ringpop-node_amd/js against the
// Python binding's timeline of the same scenario (in.json from tests/test_js_timeline_gpu.py: the
// cluster, the events, the ring capacity, the rounds to run and the expected result). Prints one
// JSON line.
'use strict';
var fs = require('fs');
var path = require('path');
var amd = require(path.join(__dirname, '..', '..', 'ringpop-node_amd', 'js'));

var input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var fails = [], checks = 0;
var sim = new amd.GossipSim(input.names, {inc0: input.inc0, dead: input.dead, seed: input.seed,
    suspicionRounds: input.suspRounds, now0: input.now0, events: input.events});
function same(what, got, want) {
    checks++;
    if (JSON.stringify(got) !== JSON.stringify(want)) { fails.push(what); }
}
same('never enabled', sim.timeline().rounds, []);
sim.timelineEnable(input.cap);
sim.step(input.rounds);
var got = sim.timeline();
same('firstRound', got.firstRound, input.want.firstRound);
same('count', got.rounds.length, input.want.rounds.length);
got.rounds.forEach(function (r, i) {
    var w = input.want.rounds[i];
    Object.keys(w).forEach(function (k) { same('round ' + w.round + ' ' + k, r[k], w[k]); });
    checks++;
    if (Object.keys(r).length !== Object.keys(w).length) { fails.push('round ' + w.round + ' fields'); }
});
checks++;
if (!(got.firstSeen instanceof Uint32Array)) { fails.push('firstSeen type'); }
same('firstSeen', Array.from(got.firstSeen), input.want.firstSeen);
sim.timelineEnable(0);
sim.step(1);
same('turned off', sim.timeline().rounds, []);
sim.destroy();
process.stdout.write(JSON.stringify({checks: checks, fails: fails.slice(0, 20), nfail: fails.length}) + '\n');
